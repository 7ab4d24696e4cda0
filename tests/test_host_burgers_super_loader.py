"""The resident pipeline of the Burgers super-resolution trainer on the CPU: pack_burgers_batch on host tensors (the index formulation) against
the present preprocess and the reference's recorded outputs, the fp64 host reference (tests/burgers_pack_ref.py) against the same recordings,
ResidentSuperBurgersLoader's contract (SuperDataLoader's: one batch of one level per iteration) with device='cpu', DiffusionDataset's lazy x
and the shared file read. The condition rows of the host formulation need this tree's GPU transforms; here the oracle's fp32 transforms stand in
for them (host_rows). The HIP launch of the same packing: tests/test_gpu_burgers_super_loader.py."""
import gc
import random
import sys

import numpy as np
import pytest
import torch

from oracle import dwt_ref as R
from tests import arbiter
from tests.burgers_pack_ref import channel_error, packed_state
from tests.helpers import load_npz

LEVELS = [(41, 60), (21, 30), (11, 15), (6, 8)]
RESC9 = torch.tensor([10, 3, 3, 1, 21, 5, 5, 1, 10]).view(1, 9, 1, 1).float()
RESC17 = torch.cat((RESC9[:, :8].repeat(1, 2, 1, 1), RESC9[:, 8:]), dim=1)
FIXTURES = (('base', 0, False, dict()), ('base_u0only', 0, False, dict(is_condition_uT=False)), ('super0', 0, True, dict()), ('super1', 1, True, dict()))


@pytest.fixture(scope='module')
def trees():
    from wdno_amd import tree_path
    for t in ('third_party', 'smoke', 'burgers'):
        p = tree_path(t)
        if p not in sys.path:
            sys.path.insert(0, p)
    return True


def oracle_rows(w_uf, shape, ori_shape, mode, wave_type):
    """_condition_rows of data_burgers_1d.py on the oracle's fp32 transforms: (lo [N, 2, nx], hi [N, 2, nx])"""
    yl, yh = R.burgers_tensor_to_coef(w_uf[:, :8].cpu().numpy(), shape)
    u = R.idwt2(yl, yh, wave_type, mode)[:, 0, :ori_shape[-2], :ori_shape[-1]]
    lo, hi = R.dwt1d(np.ascontiguousarray(u[:, [0, -1]]), wave_type, mode)
    return torch.from_numpy(lo).to(w_uf.device), torch.from_numpy(hi).to(w_uf.device)


@pytest.fixture
def host_rows(trees, monkeypatch):
    import ddpm_burgers.data_burgers_1d as DB
    monkeypatch.setattr(DB, '_condition_rows', oracle_rows)
    return DB


def golden_db():
    G = load_npz('ref_data_burgers.npz')
    coef = [torch.from_numpy(G[f'coef{i}']) for i in range(4)]
    return G, {'coef': coef, 'shape': [c.shape[2:] for c in coef], 'ori_shape': torch.Size((81, 120))}


def synthetic_db(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    coef = [torch.randn(n, 2, 4, *s, generator=g) for s in LEVELS]
    return {'coef': coef, 'shape': [c.shape[2:] for c in coef], 'ori_shape': torch.Size((81, 120))}


def ori_of(lvl):
    return [-(-81 // 2 ** lvl), -(-120 // 2 ** lvl)]


def level_datasets(DB, db, n_sets, **kw):
    return [DB.DiffusionDataset(db, preprocess=DB.get_wavelet_super_preprocess(rescaler=RESC17, is_super_model=True, N_downsample=i,
                                                                               mode='periodization', wave_type='bior2.4', **kw)) for i in range(n_sets)]


def level_of(batch):
    return {64: 0, 32: 1, 16: 2}[batch.shape[-1]]


def test_pack_batch_on_host_tensors_equals_the_preprocess(host_rows):
    """Every level of the file, base and super, all flag pairs, with and without an index list: torch.equal on all channels but the last (the
    condition channel is the stand-in's here; it is the same call in both, so it agrees too)."""
    DB = host_rows
    _, db = golden_db()
    for sup, lvl in ((False, 0), (True, 0), (True, 1), (True, 2)):
        for u0, uT in ((True, True), (True, False), (False, False)):
            resc = RESC17 if sup else RESC9
            if not (u0 or uT):
                resc = resc[:, :-1]
            pre = DB.get_wavelet_super_preprocess(rescaler=resc, is_super_model=sup, N_downsample=lvl, mode='periodization', wave_type='bior2.4',
                                                  is_condition_u0=u0, is_condition_uT=uT)
            assert pre.args['N_downsample'] == lvl and pre.args['is_condition_uT'] == uT and pre.args['rescaler'] is resc
            want, shape, ori = pre(db)
            pad = 64 // 2 ** lvl
            assert shape == list(LEVELS[lvl]) and ori == ori_of(lvl)
            fine, coarse = db['coef'][lvl], (db['coef'][lvl + 1] if sup else None)
            got = DB.pack_burgers_batch(fine, coarse, resc, ori, None, pad, pad, 'periodization', 'bior2.4', u0, uT)
            assert got.shape == want.shape and torch.equal(got[:, :-1], want[:, :-1]) and torch.equal(got, want)
            idx = [2, 0, 0]
            got = DB.pack_burgers_batch(fine, coarse, resc, ori, idx, pad, pad, 'periodization', 'bior2.4', u0, uT)
            assert torch.equal(got[:, :-1], want[idx][:, :-1])


@pytest.mark.parametrize('tag,lvl,sup,kw', FIXTURES)
def test_pack_batch_reproduces_the_reference_recorded_outputs(host_rows, tag, lvl, sup, kw):
    """out_* of tests/golden/ref_data_burgers.npz are the reference function's own outputs on these coefficients: equality on the copied channels."""
    DB = host_rows
    G, db = golden_db()
    pad = 64 // 2 ** lvl
    got = DB.pack_burgers_batch(db['coef'][lvl], db['coef'][lvl + 1] if sup else None, RESC17 if sup else RESC9, ori_of(lvl), None, pad, pad,
                                'periodization', 'bior2.4', True, kw.get('is_condition_uT', True))
    ref = G[f'out_{tag}_data']
    assert tuple(got.shape) == ref.shape and np.array_equal(got[:, :-1].numpy(), ref[:, :-1])
    assert G[f'out_{tag}_shape'].tolist() == list(LEVELS[lvl]) and G[f'out_{tag}_ori_shape'].tolist() == ori_of(lvl)


@pytest.mark.parametrize('tag,lvl,sup,kw', FIXTURES)
def test_fp64_reference_meets_the_recorded_outputs(tag, lvl, sup, kw):
    """The arbiter of the GPU gates against the recordings: the copied channels to the bit (a quotient rounded to 53 and then to 24 bits is the
    correctly rounded fp32 quotient), the condition channel inside the arbiter gate with the oracle's own fp32 evaluation as the yardstick."""
    G, db = golden_db()
    pad = 64 // 2 ** lvl
    a = (db['coef'][lvl].numpy(), db['coef'][lvl + 1].numpy() if sup else None, (RESC17 if sup else RESC9).reshape(-1).numpy(), ori_of(lvl), pad, pad)
    flags = dict(u0=True, uT=kw.get('is_condition_uT', True))
    exact, f32 = packed_state(*a, **flags), packed_state(*a, dtype=np.float32, **flags)
    ref = G[f'out_{tag}_data']
    assert np.array_equal(exact[:, :-1].astype(np.float32), ref[:, :-1])
    e_ref, e_f32 = channel_error(ref[:, -1], exact[:, -1]), channel_error(f32[:, -1], exact[:, -1])
    print(f'{tag}: condition channel vs fp64 -- recorded {e_ref:.3e}, fp32 oracle {e_f32:.3e}')
    assert e_ref < 1e-6 and arbiter.gate(e_ref, e_f32)
    if not flags['uT']:
        assert not exact[:, -1, pad // 2:].any() and exact[:, -1, :pad // 2, :LEVELS[lvl][1]].any()


def test_resident_loader_contract_on_the_host(host_rows):
    """One batch per __iter__, each the items of its level's dataset bit for bit; per level every epoch is a permutation with the short last batch
    kept and reshuffled; the level sequence is random.Random(seed)'s; the levels are held once each."""
    DB = host_rows
    from wdno_amd.loader import ResidentSuperBurgersLoader
    n = 5
    db = synthetic_db(n)
    sets = level_datasets(DB, db, 3)
    ld = ResidentSuperBurgersLoader(sets, 2, 'cpu', seed=11, order_seed=3)
    assert all(ds._x is None for ds in sets)                       # the loader packs from the levels: no dataset has built its tensor
    assert len(ld) == 3 * 3 and ld.resident_bytes() == 4 * n * 8 * sum(a * b for a, b in LEVELS)
    seen, sizes, levels = [[], [], []], [[], [], []], []
    for _ in range(30):
        batches = list(ld)
        assert len(batches) == 1                                   # SuperDataLoader's contract
        lvl, ids = ld.last_ids
        assert level_of(batches[0]) == lvl and batches[0].shape == (len(ids), 17, 64 >> lvl, 64 >> lvl)
        assert torch.equal(batches[0], sets[lvl].x[ids])
        levels.append(lvl)
        seen[lvl] += ids
        sizes[lvl].append(len(ids))
    r = random.Random(11)
    assert levels == [r.randint(0, 2) for _ in range(30)]
    for lvl in range(3):
        assert len(seen[lvl]) >= 2 * n                             # (seed 11: every level completes two epochs within 30 draws)
        for k in range(0, len(seen[lvl]) - n + 1, n):
            assert sorted(seen[lvl][k:k + n]) == list(range(n))
        assert sizes[lvl][:3] == [2, 2, 1] and seen[lvl][:n] != seen[lvl][n:2 * n]
    assert ld.samplers[0].indices() != ld.samplers[1].indices()


def test_resident_loader_shards_and_input_checks(host_rows):
    """Two ranks walk disjoint shards of each level's epoch (DistributedSampler's rule, the permutation seed offset by the level) and draw the same
    level at every step; anything but the levels 0 .. N - 1 of one file with one set of flags is refused."""
    DB = host_rows
    from torch.utils.data.distributed import DistributedSampler
    from wdno_amd.loader import ResidentSuperBurgersLoader
    n = 6
    db = synthetic_db(n, seed=1)
    sets = level_datasets(DB, db, 2, is_condition_uT=False)
    a = ResidentSuperBurgersLoader(sets, 2, 'cpu', rank=0, world=2, seed=5, order_seed=0)
    b = ResidentSuperBurgersLoader(sets, 2, 'cpu', rank=1, world=2, seed=5, order_seed=0)
    drawn = {0: ([], []), 1: ([], [])}
    for _ in range(12):
        list(a), list(b)
        assert a.last_ids[0] == b.last_ids[0]
        drawn[a.last_ids[0]][0].extend(a.last_ids[1])
        drawn[a.last_ids[0]][1].extend(b.last_ids[1])
    for lvl in (0, 1):
        da, db_ = drawn[lvl]
        assert len(da) >= 3 and not set(da[:3]) & set(db_[:3]) and sorted(da[:3] + db_[:3]) == list(range(n))
        s = DistributedSampler(sets[lvl], num_replicas=2, rank=0, shuffle=True, seed=lvl)
        s.set_epoch(0)
        assert list(s) == da[:3]
    base = DB.DiffusionDataset(db, preprocess=DB.get_wavelet_super_preprocess(rescaler=RESC9, mode='periodization', wave_type='bior2.4'))
    other = level_datasets(DB, synthetic_db(n, seed=2), 2, is_condition_uT=False)
    mixed = [sets[0], level_datasets(DB, db, 2)[1]]
    for bad in ([base], sets[1:], [sets[0], other[1]], mixed, [], level_datasets(DB, db, 4)):
        with pytest.raises(ValueError):
            ResidentSuperBurgersLoader(bad, 2, 'cpu')


def test_level_datasets_build_x_on_first_use(host_rows):
    DB = host_rows
    _, db = golden_db()
    calls = []
    pre = DB.get_wavelet_super_preprocess(rescaler=RESC17, is_super_model=True, N_downsample=1, mode='periodization', wave_type='bior2.4')
    counted = lambda d: (calls.append(1), pre(d))[1]
    counted.args = pre.args
    ds = DB.DiffusionDataset(db, preprocess=counted)
    assert not calls and len(ds) == ds.len() == 3 and ds.shape == [21, 30] and ds.ori_shape == [41, 60]
    item = ds[0]
    assert len(calls) == 1 and item.shape == (17, 32, 32)
    assert torch.equal(ds.x, pre(db)[0]) and torch.equal(ds.get(2), ds.x[2]) and len(calls) == 1
    ds2 = DB.DiffusionDataset(db, preprocess=counted)
    DB.SuperDataLoader([ds2], batch_size=2, num_workers=0, pin_memory=False)
    assert len(calls) == 2 and ds2._x is not None
    ds3 = DB.DiffusionDataset(db, preprocess=counted)
    monkey_info = torch.utils.data.get_worker_info
    torch.utils.data.get_worker_info = lambda: object()             # as seen from inside a DataLoader worker
    try:
        with pytest.raises(RuntimeError, match='in the parent'):
            ds3[0]
    finally:
        torch.utils.data.get_worker_info = monkey_info
    # base datasets stay eager
    calls.clear()
    pre0 = DB.get_wavelet_super_preprocess(rescaler=RESC9, mode='periodization', wave_type='bior2.4')
    eager = lambda d: (calls.append(1), pre0(d))[1]
    eager.args = pre0.args
    ds0 = DB.DiffusionDataset(db, preprocess=eager)
    assert len(calls) == 1 and ds0.x.shape == (3, 9, 64, 64) and ds0.shape == [41, 60] and ds0.ori_shape == [81, 120]


def test_a_coefficient_file_is_read_once_for_its_level_datasets(host_rows, tmp_path, monkeypatch):
    DB = host_rows
    import os
    _, db = golden_db()
    path = str(tmp_path / 'coef_bior2.4_periodization_super')
    torch.save(db, path)
    loads = []
    real = torch.load
    monkeypatch.setattr(torch, 'load', lambda *a, **k: (loads.append(a[0]), real(*a, **k))[1])
    sets = level_datasets(DB, path, 3)
    assert loads == [path] and all(d.db is sets[0].db for d in sets)
    assert [d.shape for d in sets] == [list(s) for s in LEVELS[:3]] and torch.equal(sets[2].x, level_datasets(DB, db, 3)[2].x)
    os.utime(path, (1, 1))                                         # another mtime: the file is read again
    assert DB.DiffusionDataset(path, preprocess=sets[0].preprocess).db is not sets[0].db and len(loads) == 2
    del sets                                                       # the shared dictionary lives as long as a dataset holds it, no longer
    gc.collect()
    assert path not in DB._files
