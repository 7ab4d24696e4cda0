"""wdno_pack_smoke_super_state (csrc/pack.hip) against the host index formulation that tests/test_host_super_loader.py pins to Smoke_wave's items
and to the reference's recorded states, ResidentSuperSmokeLoader on the device, and the smoke Trainer picking it up for a list of level datasets."""
import math
import random
import sys

import numpy as np
import pytest
import torch

from tests.test_host_super_loader import LEVEL_SHAPES, golden_levels, level_datasets, level_of, super_files

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def trees():
    from wdno_amd import tree_path
    for t in ('third_party', 'smoke', 'burgers'):
        p = tree_path(t)
        if p not in sys.path:
            sys.path.insert(0, p)
    return True


def _stores(kind, nf, nt, nx, n=6, seed=1):
    from ddpm.data_2d import _RESCALERS
    g = torch.Generator().manual_seed(seed)
    nt_c, nx_c = ((nt + 2) // 2, nx) if kind == 'time' else (nt, (nx + 2) // 2)
    fine = torch.randn(n, nf, 8, nt, nx, nx, generator=g)
    coarse = torch.randn(n, nf, 8, nt_c, nx_c, nx_c, generator=g)
    init5 = torch.randn(n, 5, 4, nx, nx, generator=g)
    so = torch.rand(n, 2, nt, generator=g)
    r = torch.tensor(_RESCALERS['bior1.3'], dtype=torch.float32)
    r = torch.cat((r[:8 * nf], r[40 - 8 * nf:40], r[-2:]))            # (nf = 5: Smoke_wave's RESCALER of the super-resolution models)
    return fine, coarse, init5, so, r


CASES = [('time', 5, 18, 34, 24, 40),       # the real level 0
         ('time', 5, 10, 34, 12, 40),       # the real level 1
         ('space', 5, 18, 34, 24, 40),      # the real level 0
         ('space', 5, 18, 18, 24, 20),      # the real level 1
         ('time', 2, 2, 7, 4, 8),           # the box fills pad_t, odd rows: no 8-byte loads
         ('time', 2, 2, 6, 8, 8),           # zero frames after the box
         ('space', 2, 3, 6, 4, 8),          # nx + 2 == pad_x: no zero columns
         ('space', 1, 4, 2, 4, 8)]          # nx = 2: every fine column touches a clamp


@pytest.mark.parametrize('kind,nf,nt,nx,pad_t,pad_x', CASES)
def test_pack_super_kernel_is_bit_identical_to_the_index_formulation(trees, kind, nf, nt, nx, pad_t, pad_x):
    """torch.equal (IEEE division in both) with and without an index list into six resident simulations, for both layouts of the initial
    coefficients."""
    from ddpm.data_2d import pack_smoke_super_batch, pack_smoke_super_gpu
    fine, coarse, init5, so, r = _stores(kind, nf, nt, nx)
    want = pack_smoke_super_batch(fine, coarse, init5, so, r, kind, None, pad_t, pad_x)             # host tensors: the index formulation
    assert want.shape == (6, pad_t, 16 * nf + 2, pad_x, pad_x)
    d = [t.to(DEV) for t in (fine, coarse, init5, so)]
    init4 = init5[:, 0].contiguous().to(DEV)
    pick = [4, 0, 0, 5]
    idx = torch.tensor(pick, device=DEV)
    for init in (d[2], init4):
        got = pack_smoke_super_batch(d[0], d[1], init, d[3], r.to(DEV), kind, None, pad_t, pad_x)
        assert got.is_cuda and torch.equal(got.cpu(), want)
        got = pack_smoke_super_gpu(d[0], d[1], init, d[3], r, kind, idx, pad_t, pad_x)
        assert torch.equal(got.cpu(), want[pick])


@pytest.mark.parametrize('kind', ['time', 'space'])
def test_pack_super_kernel_reproduces_the_reference_recorded_states(trees, kind):
    from ddpm.data_2d import pack_smoke_super_gpu
    fine, coarse, init5, so, resc, want = golden_levels(kind)
    got = pack_smoke_super_gpu(fine.to(DEV), coarse.to(DEV), init5.to(DEV), so.to(DEV), resc, kind)
    assert np.array_equal(got[0].cpu().numpy(), want)


def test_pack_super_shape_rules_return_a_code_without_a_launch(trees):
    """WDNO_EINVAL (-1) / WDNO_EUNSUPPORTED (-3) from the entry itself, the state left as it was; the Python launch raises."""
    from wdno_amd.ops import _lib_, _p, _stream
    from ddpm.data_2d import pack_smoke_super_gpu
    lib = _lib_()
    buf = torch.zeros(1 << 16, device=DEV)
    out = torch.full((1 << 16,), 7.0, device=DEV)

    def call(kind, nt, nx, nt_c, nx_c, pad_t, pad_x):
        return lib.wdno_pack_smoke_super_state(_p(buf), 8 * nt * nx * nx, _p(buf), 8 * nt_c * nx_c * nx_c, _p(buf), 4 * nx * nx, _p(buf), 2 * nt, None,
                                               _p(buf), _p(out), 1, 1, nt, nx, nt_c, nx_c, kind, pad_t, pad_x, _stream())
    assert call(0, 2, 6, 2, 6, 4, 8) == 0                          # (the calls below differ from a valid one in one number each)
    out.fill_(7.0)
    assert call(0, 2, 6, 3, 6, 8, 8) == -1                         # nt + 2 != 2 nt_c
    assert call(1, 4, 6, 4, 3, 4, 8) == -1                         # nx + 2 != 2 nx_c
    assert call(0, 2, 5, 2, 5, 4, 6) == -3                         # pad_x % 4 != 0
    assert call(0, 2, 6, 2, 6, 6, 8) == -3                         # pad_t % 4 != 0
    assert call(1, 4, 6, 4, 4, 4, 4) == -1                         # nx + 2 > pad_x
    assert call(0, 6, 6, 4, 6, 4, 8) == -1                         # nt + 2 > pad_t
    assert call(2, 2, 6, 2, 6, 4, 8) == -1                         # no such kind
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    fine, coarse, init5, so, r = (t.to(DEV) for t in _stores('time', 1, 2, 6))
    with pytest.raises(RuntimeError, match='invalid argument'):
        pack_smoke_super_gpu(fine, coarse, init5, so, r, 'time', None, 8, 4)
    with pytest.raises(RuntimeError, match='contiguous float32'):
        pack_smoke_super_gpu(fine.cpu(), coarse, init5, so, r, 'time', None, 4, 8)


@pytest.mark.parametrize('kind', ['time', 'space'])
def test_a_sample_has_the_same_bits_alone_and_inside_a_larger_batch(trees, kind):
    from ddpm.data_2d import pack_smoke_super_gpu
    nt, nx, pad_t, pad_x = (10, 34, 12, 40) if kind == 'time' else (18, 18, 24, 20)
    fine, coarse, init5, so, r = (t.to(DEV) for t in _stores(kind, 5, nt, nx, seed=2))
    one = pack_smoke_super_gpu(fine, coarse, init5, so, r, kind, torch.tensor([3], device=DEV), pad_t, pad_x)
    many = pack_smoke_super_gpu(fine, coarse, init5, so, r, kind, torch.tensor([1, 5, 3, 2, 3], device=DEV), pad_t, pad_x)
    assert torch.equal(one[0], many[2]) and torch.equal(one[0], many[4])


@pytest.mark.parametrize('kind', ['time', 'space'])
def test_resident_super_loader_on_the_device_equals_the_datasets(trees, tmp_path, kind):
    """Two epochs per level of 11 simulations with N = 2: every batch equals the items of its level's dataset bit for bit, every epoch of a level is
    a permutation, the files are read once."""
    from wdno_amd.loader import ResidentSuperSmokeLoader
    n = 11
    super_files(tmp_path, kind, n, 3)
    sets = level_datasets(tmp_path, kind, 2, n)
    loads = []
    for ds in sets:
        ds.raw_levels = (lambda s, k, _f=ds.raw_levels: (loads.append(s), _f(s, k))[1])
    want = [[ds[i][0] for i in range(n)] for ds in sets]          # the reference once, shared by every batch below
    ld = ResidentSuperSmokeLoader(sets, 4, DEV, seed=2, order_seed=5, num_workers=0)
    seen = [[], []]
    for _ in range(200):
        if min(len(s) for s in seen) >= 2 * n:
            break
        (state, shape, _, ids), = list(ld)
        lvl = level_of(state, kind)
        assert state.is_cuda and shape == list(LEVEL_SHAPES[kind][lvl])
        host = state.cpu()
        for j, i in enumerate(ids.tolist()):
            assert torch.equal(host[j], want[lvl][i])
        seen[lvl] += ids.tolist()
    for lvl in range(2):
        assert len(seen[lvl]) >= 2 * n and min(ld.epoch) >= 1
        for k in range(0, len(seen[lvl]) - n + 1, n):
            assert sorted(seen[lvl][k:k + n]) == list(range(n))
    assert sorted(loads) == list(range(n))
    assert ld.resident_bytes() == n * sum(4 * (40 * s[0] * s[1] * s[2] + 4 * s[1] * s[2] + 2 * s[0]) for s in LEVEL_SHAPES[kind])


def test_smoke_trainer_picks_the_resident_super_loader(trees, tmp_path):
    """A smoke Trainer on a list of two level datasets (time variant: states [B, 24, 82, 40, 40] and [B, 12, 82, 40, 40]) gets the resident loader and
    steps across both levels; with resident_data off it gets SuperDataLoader as before."""
    from ddpm.data_2d import SuperDataLoader
    from ddpm.diffusion_2d import GaussianDiffusion, Trainer
    from video_diffusion_pytorch.video_diffusion_pytorch_conv3d import Unet3D_with_Conv3D
    from wdno_amd.loader import ResidentSuperSmokeLoader
    from wdno_amd.trainer import TrainerCore
    n = 4
    super_files(tmp_path, 'time', n, 3)
    sets = level_datasets(tmp_path, 'time', 2, n)
    torch.manual_seed(0)
    net = Unet3D_with_Conv3D(dim=8, dim_mults=(1, 2), channels=82, resnet_groups=4, init_kernel_size=3)
    dif = GaussianDiffusion(net, torch.ones(1, 1, 82, 1, 1), False, True, True, True, 'bior1.3', 'zero', [[18, 34, 34], [10, 34, 34]], None,
                            image_size=40, frames=24, timesteps=1000, sampling_timesteps=10, loss_type='l2')
    seed = next(s for s in range(100) if len(set(_draws(s, 3))) == 2)      # a level sequence of the global `random` that meets both levels in three steps
    prev = TrainerCore.num_workers
    TrainerCore.num_workers = 0
    try:
        tr = Trainer(dif, sets, None, train_batch_size=2, train_lr=1e-3, train_num_steps=3, results_path=str(tmp_path / 'a'), calculate_fid=False)
        ld = tr.dl.gi_frame.f_locals['dl']
        assert isinstance(ld, ResidentSuperSmokeLoader)
        random.seed(seed)
        shapes = []
        w0 = tr.opt.buf.flat_param.clone()
        for _ in range(3):
            batch = {}
            loss = tr.optimisation_step(lambda: batch.setdefault('x', tr._next_state()))
            assert batch['x'].is_cuda and math.isfinite(loss)
            shapes.append(tuple(batch['x'].shape))
        assert set(shapes) == {(2, 24, 82, 40, 40), (2, 12, 82, 40, 40)}
        assert (tr.opt.buf.flat_param - w0).abs().max() > 0 and bool(torch.isfinite(tr.opt.buf.flat_param).all())
        assert ld.resident_bytes() > 0

        class NoRes(Trainer):
            resident_data = False
        tr2 = NoRes(dif, sets, None, train_batch_size=2, train_num_steps=3, results_path=str(tmp_path / 'b'), calculate_fid=False)
        assert isinstance(tr2.dl.gi_frame.f_locals['dl'], SuperDataLoader)
        assert tuple(next(tr2.dl)[0].shape[2:]) == (82, 40, 40)
    finally:
        TrainerCore.num_workers = prev
    torch.cuda.synchronize()


def _draws(seed, k):
    r = random.Random(seed)
    return [r.randint(0, 1) for _ in range(k)]

