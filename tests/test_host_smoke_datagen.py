"""Host side of the smoke data-set generator (wdno_amd/smoke_datagen.py) and its test infrastructure (tests/smoke_datagen_ref.py): the
scene sampler against the reference fixtures, plan(), the Philox4x32-10 restatement against the Random123 known answers, the statistics
of the seeded noise, the numpy restatement of the loop against the reference's records, and the file layout. No GPU."""
import os

import numpy as np
import pytest

from tests import smoke_datagen_ref as RD

G, M = RD.load_golden()
CASES = sorted(M['cases'])


@pytest.mark.parametrize('name', CASES)
def test_sample_scenes_equals_the_reference_scene(name):
    from wdno_amd.smoke_datagen import kick_frames, sample_scenes
    c = M['cases'][name]
    sc = sample_scenes([0], c['seed'], c['scenelength'])
    for k in ('xs', 'ys', 'vxs', 'vys', 'intervals'):
        assert sc[k][0].tolist() == c['scene'][k], k                     # exactly: the floats are the reference's doubles
    assert kick_frames(sc['intervals'])[0].tolist() == c['kick_frames']
    # scene i of data set `seed` is scene 0 of data set seed + i; the replay of the test infrastructure agrees
    assert sample_scenes([3], c['seed'] - 3, c['scenelength'])['vxs'][0].tolist() == c['scene']['vxs']
    assert RD.replay_scene(np.random.RandomState(c['seed']), c['scenelength']) == c['scene']


def test_fixture_cases_are_the_ones_the_tests_rely_on():
    assert M['cases']['short_a']['kick_frames'] == [0, 5, 8, 14] and M['cases']['short_b']['kick_frames'] == [0, 5, 9, 15]
    assert M['cases']['full']['kick_frames'] == [0, 42, 74, 128]
    assert 8 in M['cases']['short_a']['kick_frames']                     # a kick on a record frame
    assert sum(bool(M['cases'][n]['smoke_in_buckets']) for n in CASES) >= 2
    sm = G['short_b/smoke']
    assert 0 < sm[3, 1] < 1e-6 and 4e-3 < sm[4, 1] < 6e-3               # bucket 1 receives smoke by record 3
    assert (M['cases']['short_b_t64']['record_scale'], M['cases']['short_b_t64']['stride']) == (1, 2)
    assert (M['cases']['short_b_t128']['record_scale'], M['cases']['short_b_t128']['stride']) == (8, 1)


def test_plan_kick_frames_and_errors():
    from wdno_amd.smoke_datagen import plan, sample_scenes
    sc = sample_scenes([0, 1, 2], 0, 32)
    pl = plan(sc)
    assert pl['kick_frames'][0].tolist() == [0, 5, 8, 14] and pl['records'] == 5 and pl['n'] == 64 and pl['B'] == 3
    assert plan(sc, record_scale=1)['records'] == 33 and plan(sc, stride=1)['n'] == 128
    assert plan(sample_scenes([0], 5, 256))['records'] == 33
    assert plan(sc, threads=1024)['threads'] == 1024
    for kw in (dict(record_scale=0), dict(stride=3), dict(stride=0), dict(threads=256)):
        with pytest.raises(ValueError):
            plan(sc, **kw)
    for S in (0, 257):
        with pytest.raises(ValueError):
            plan(dict(sc, scenelength=S))
    bad = dict(sc, intervals=sc['intervals'].copy())
    bad['intervals'][1, 1] = 0
    with pytest.raises(ValueError, match='interval'):
        plan(bad)


def test_generate_wants_exactly_one_noise_source():
    from wdno_amd.smoke_datagen import generate, sample_scenes
    sc = sample_scenes([0], 0, 32)
    with pytest.raises(ValueError):
        generate(sc)
    with pytest.raises(ValueError):
        generate(sc, seed=1, noise=np.zeros((1, 33, 128, 128, 2)))


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10."""
    pi = [0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344]
    for ctr, key, want in (([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
                           ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
                           (pi, [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])):
        got = RD.philox4x32_10(np.array(ctr, np.uint32), np.array(key, np.uint32))
        assert got.tolist() == want
    both = RD.philox4x32_10(np.array([[0] * 4, pi], np.uint32), np.array([[0, 0], [0xa4093822, 0x299f31d0]], np.uint32))
    assert both[1].tolist() == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1] and both[0, 0] == 0x6627e8d5


def test_seeded_noise_statistics():
    """Unit normals of the rim cells over 64 frames of one scene: N = 64 * 7168 * 2 ~ 9.2e5 draws at fixed seeds. The bounds are five
    standard errors of the estimators under the hypothesis (1 / sqrt(N) for a mean and a correlation, sqrt(2 / N) for a variance)."""
    rim = np.ones((128, 128), bool)
    rim[16:112, 16:112] = False
    seed = 20240607
    z = np.stack([RD.unit_normals(seed, 12, f)[rim] for f in range(64)]).astype(np.float64)        # [64, 7168, 2]
    other = np.stack([RD.unit_normals(seed, 13, f)[rim] for f in range(64)]).astype(np.float64)
    N = z.size
    assert N == 64 * 7168 * 2
    assert np.isfinite(z).all() and np.abs(z).max() < 5.78                  # sqrt(-2 ln 2^-24) = 5.768
    assert abs(z.mean()) < 5 / np.sqrt(N)
    assert abs(z.var() - 1) < 5 * np.sqrt(2 / N)
    corr = lambda a, b: float(np.mean(a * b))
    assert abs(corr(z[:-1], z[1:])) < 5 / np.sqrt(z[1:].size)               # consecutive frames
    assert abs(corr(z, other)) < 5 / np.sqrt(N)                              # scenes i and i + 1
    assert abs(corr(z[..., 0], z[..., 1])) < 5 / np.sqrt(N / 2)              # the two components of a cell
    f = RD.noise_field(seed, 12, 3)
    assert f.dtype == np.float32 and np.array_equal(f, np.float32(0.1) * RD.unit_normals(seed, 12, 3))
    k = RD.noise_field(seed, 12, 3, (0.5, -2.0))
    assert abs(float(k[..., 0].mean()) - 0.5) < 5 * 0.05 / 128 and abs(float(k[..., 1].mean()) + 2.0) < 5 * 0.2 / 128


def test_restatement_reproduces_short_a_bit_for_bit():
    """The fp32 restatement on the replayed draws against the reference's records of case short_a (5 records of a 32-frame scene)."""
    from wdno_amd.smoke_solver import geometry
    c = M['cases']['short_a']
    scene, noise = RD.replay(c['seed'], c['scenelength'])
    assert scene == c['scene']
    out = RD.generate(geometry(), scene, noise, c['scenelength'], c['record_scale'], c['stride'])
    for k in ('density', 'velocity', 'control'):
        assert out[k].dtype == np.float32 and np.array_equal(out[k], G[f'short_a/{k}']), k
    # column 7 is an fp32 np.sum in the reference, an fp64 sum here; the bucket columns are fp64 sums in both
    assert np.array_equal(out['smoke'][:, :7], G['short_a/smoke'][:, :7])
    assert np.allclose(out['smoke'][:, 7], G['short_a/smoke'][:, 7], rtol=1e-6, atol=0)
    assert np.array_equal(out['velocity'][0, ..., 0], out['velocity'][0, ..., 1])          # the reference's record 0


@pytest.mark.parametrize('split, R, n', [('train', 33, 64), ('test_64', 257, 64), ('test_128', 33, 128)])
def test_file_layout_is_read_back_by_the_loader_rules(tmp_path, split, R, n):
    """write_sim's files hold the reference's shapes and dtype, and read_sim -- Smoke.__getitem__'s permutes, share and [:, :32] -- gives
    [32, 6, n, n] with each channel where the loader expects it. Stub arrays; no GPU."""
    from wdno_amd import smoke_datagen as GEN
    assert GEN.plan(GEN.sample_scenes([0], 5, 256), GEN.SPLITS[split]['record_scale'], GEN.SPLITS[split]['stride'])['records'] == R
    rng = np.random.default_rng(0)
    density = rng.random((R, n, n), np.float32)
    velocity, control = rng.random((R, n, n, 2), np.float32), rng.random((R, n, n, 2), np.float32)
    smoke = rng.random((R, 8)) + 0.1
    domain = np.ones((1, 127, 127, 1), np.int8)
    root = os.path.join(str(tmp_path), GEN.SPLITS[split]['dir'])
    for i, dtype in ((7, np.float64), (8, np.float32)):
        GEN.write_sim(GEN.sim_dir(root, i), density, velocity, control, smoke, domain, dtype)
        path = os.path.join(root, f'sim_{i:06d}')
        assert sorted(os.listdir(path)) == ['Control.npy', 'Density.npy', 'Smoke.npy', 'Velocity.npy', 'domain.npy', 'smoke_out.csv']
        D, V, C, S = (np.load(os.path.join(path, f + '.npy')) for f in ('Density', 'Velocity', 'Control', 'Smoke'))
        assert D.shape == (n, n, 1, R) and V.shape == C.shape == (n, n, 2, R) and S.shape == (R, 8)
        assert D.dtype == V.dtype == C.dtype == dtype and S.dtype == np.float64
        assert np.load(os.path.join(path, 'domain.npy')).shape == (1, 127, 127, 1)
        assert np.allclose(np.loadtxt(os.path.join(path, 'smoke_out.csv'), delimiter=','), smoke)
        state = GEN.read_sim(root, i).numpy()
        assert state.shape == (32, 6, n, n) and state.dtype == np.float32
        assert np.array_equal(state[:, 0], density[:32]) and np.array_equal(state[:, 1], velocity[:32, ..., 0])
        assert np.array_equal(state[:, 2], velocity[:32, ..., 1]) and np.array_equal(state[:, 3], control[:32, ..., 0])
        assert np.array_equal(state[:, 4], control[:32, ..., 1])
        share = (smoke[:, 1].astype(np.float32) / smoke.astype(np.float32).sum(-1))[:32]
        assert np.allclose(state[:, 5], share[:, None, None], rtol=1e-6)


def test_script_scene_ranges_are_the_reference_ones():
    from wdno_amd.smoke_datagen import branch_scenes
    assert list(branch_scenes('train', True, False, '3')) == [6, 7] and list(branch_scenes('train', False, True, 1)) == [5, 6, 7, 8, 9]
    assert list(branch_scenes('test_64', False, True, 2)) == list(range(20, 30)) and len(branch_scenes('test_64', True, False, 0)) == 5
    assert len(branch_scenes('test_128', True, False, 0)) == 40 and len(branch_scenes('test_128', False, True, 0)) == 5
    assert len(branch_scenes('train', False, False, 0)) == 40
