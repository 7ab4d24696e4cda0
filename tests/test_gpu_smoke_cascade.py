"""The smoke super-resolution cascade on the GPU: csrc/smoke_cascade.hip, the offset entry of csrc/smoke_reconstruct.hip and the four-way entry
of csrc/smoke_score.hip through wdno_amd/smoke/cascade.py, reconstruct.py, score.py and the driver wdno_amd/smoke/inference_2d.py, against
what the reference's own run_model -> run_super_model and multi_evaluate produced (tests/golden/ref_smoke_cascade_*.npz, inputs regenerated
by tests/smoke_cascade_inputs.py), fp64 evaluations (oracle/dwt_ref.py, plain numpy) and the existing routes. GPU box only.

Gates. Conditions: index work bit-equal to the CPU route, transforms 1e-6 relative max-abs against the reference run (the bar of the base
conditions in tests/test_gpu_smoke_inference.py). Reconstruction: tests.arbiter.gate with factor 1.5 and slack 1e-6 against the exact value
that tests/test_host_smoke_cascade.py pins to the reference's fp64 run. Scores: the score gate of tests/test_gpu_smoke_inference.py
(A.gate(hip_err, ref_err, factor=1.0, slack=1e-12)) against the numpy fp64 evaluation. Identical bits wherever the same launch runs twice."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import arbiter as A
from tests import smoke_cascade_inputs as SC
from tests.helpers import GOLDEN, load_npz
from tests.test_host_smoke_cascade import check_conditions, cpu_conditions

pytestmark = pytest.mark.gpu
DEV = 'cuda'
with open(os.path.join(GOLDEN, 'ref_smoke_cascade_manifest.json')) as _f:
    MAN = json.load(_f)
W_E = MAN['w_energy']
REF_KEYS = (('J_total', 'J_total'), ('J_target', 'J_target'), ('J_energy', 'J_energy'), ('mse', 'mse_wo_smoke'), ('n_l2', 'n_l2'))


@pytest.fixture(scope='module')
def trees():
    from wdno_amd import tree_path
    for t in ('third_party', 'smoke'):
        p = tree_path(t)
        if p not in sys.path:
            sys.path.insert(0, p)
    import inference_2d as INF
    from video_diffusion_pytorch.video_diffusion_pytorch_conv3d import Unet3D_with_Conv3D
    from ddpm.diffusion_2d import GaussianDiffusion
    from wdno_amd.smoke import cascade as Cs, guidance as Gd, reconstruct as Rc, score as Sc
    return dict(INF=INF, Cs=Cs, Rc=Rc, Sc=Sc, Gd=Gd, Unet3D=Unet3D_with_Conv3D, GD=GaussianDiffusion)


def _relmax(a, e):
    return float(np.abs(a - e).max() / np.abs(e).max())


def _gpu_conditions(Cs, name, prev=None, fine=None):
    c = SC.CASES[name]
    prev = SC.sample_output(name, 0).to(DEV) if prev is None else prev
    fine = SC.fine_state(name).to(DEV) if fine is None else fine
    return Cs.super_conditions(prev, c['shape'][0], fine, SC.rescaler().to(DEV), c['shape'][1], SC.PAD_T, SC.PAD_X)


# ----------------------------------------------------------------------------------------------------- conditions
@pytest.mark.parametrize('name', sorted(SC.CASES))
def test_conditions_kernel_against_the_cpu_route_and_the_reference(trees, name):
    Cs = trees['Cs']
    src = _gpu_conditions(Cs, name)
    assert src.is_cuda and src.is_contiguous()
    ei, ec = check_conditions(src.cpu(), name, Cs.views)
    print(f'{name}: init {ei:.3e}, control {ec:.3e} (relative max-abs against the reference run)')
    assert ei <= 1e-6 and ec <= 1e-6, (ei, ec)
    cpu, got = cpu_conditions(Cs, name), src.cpu()
    assert torch.equal(got[:, :, 40:80], cpu[:, :, 40:80]) and torch.equal(got[:, :, :24], cpu[:, :, :24]) and torch.equal(got[:, :, -1], cpu[:, :, -1])
    e = float((got - cpu).abs().max() / cpu.abs().max())
    print(f'{name}: GPU against the CPU route {e:.3e}')
    assert e <= 1e-6


def test_conditions_batch_invariance_and_strided_views(trees):
    Cs, name = trees['Cs'], 'small'
    prev, fine = SC.sample_output(name, 0), SC.fine_state(name)
    p3, f3 = torch.cat((prev, prev[:1] * 0.5)).to(DEV), torch.cat((fine, fine[:1] * 0.5)).to(DEV)
    all3 = _gpu_conditions(Cs, name, p3, f3)
    assert torch.equal(all3[:2], _gpu_conditions(Cs, name))
    for b in range(3):
        assert torch.equal(_gpu_conditions(Cs, name, p3[b:b + 1], f3[b:b + 1]), all3[b:b + 1]), b
        assert torch.equal(_gpu_conditions(Cs, name, p3[b:b + 1].clone(), f3[b:b + 1].clone()), all3[b:b + 1]), b
    wide = torch.randn(5, 26, 84, 40, 48, device=DEV)                                       # the sample as a view: samples 1..3, frames 1..24, channels 2 c
    view = wide[1:4, 1:25, ::2, :, :40]
    view.copy_(p3)
    assert not view.is_contiguous() and view.stride(2) == 2 * 40 * 48
    assert torch.equal(_gpu_conditions(Cs, name, view, f3), all3)
    bigf = torch.randn(3, 16, 8, 64, 72, device=DEV)                                         # the fine state as a view with wider rows
    fview = bigf[:, :, 1:7, :, :64]
    fview.copy_(f3)
    assert torch.equal(_gpu_conditions(Cs, name, p3, fview), all3)


# ----------------------------------------------------------------------------------------------------- reconstruction
_exact = {}


def _level(name, level):
    """(x, the level's rescaler, block, field size, split row, upsample_type, exact pred); the exact value is computed once and shared."""
    c = SC.CASES[name]
    shape, ori, half = c['shape'][level], c['ori'][level], 20 * 2 ** level
    if (name, level) not in _exact:
        x, r = SC.sample_output(name, level), SC.level_rescaler(level)
        _exact[name, level] = (x, r, SC.exact_pred(x, r, shape, ori, half, level))
    x, r, e = _exact[name, level]
    return x, r, shape, ori, half, ('space' if level else None), e


@pytest.mark.parametrize('level', [0, 1])
@pytest.mark.parametrize('name', sorted(SC.CASES))
def test_reconstruct_level_under_arbiter_gate(trees, name, level):
    x, r, shape, ori, half, up, e = _level(name, level)
    g = load_npz(SC.FILE_PRED(name, level))
    ref = g['ref_err']
    pred = trees['Rc'].reconstruct(x.to(DEV), shape, ori, r.to(DEV), upsample_type=up, half=half)
    assert pred.dtype == torch.float32 and tuple(pred.shape) == e.shape and pred.is_contiguous()
    p = pred.double().cpu().numpy()
    h04, h5, r04, r5 = _relmax(p[:, :, :5], e[:, :, :5]), _relmax(p[:, :, 5], e[:, :, 5]), ref[0] / ref[1], ref[2] / ref[3]
    print(f'{name} level {level}: channels 0..4 hip {h04:.3e} reference {r04:.3e}; channel 5 hip {h5:.3e} reference {r5:.3e}')
    assert A.gate(h04, r04, factor=1.5, slack=1e-6), (h04, r04)
    assert A.gate(h5, r5, factor=1.5, slack=1e-6), (h5, r5)
    assert float((pred[:, :, 5] - pred[:, :, 5, :1, :1]).abs().max()) == 0.0          # one value per frame in every cell
    # against the reference's own fp32 entries: both are within their errors of the exact value
    s04 = _relmax(p[:, SC.PRED_FRAMES(ori[0]), :5, ::SC.PRED_ROWS], g['pred04'].astype(np.float64))
    s5 = _relmax(p[:, :, 5, 0, 0], g['pred5'].astype(np.float64))
    assert s04 <= 2.5 * r04 + 1e-6 and s5 <= 2.5 * r5 + 1e-6, (s04, s5)


def test_reconstruct_wrong_offset_or_split_row_is_caught_by_the_fixture(trees):
    """Level 1 with the block at offset 0, or the rows split at 20 (_split_row's value), is far from the reference's stored values."""
    name = 'small'
    x, r, shape, ori, half, up, _ = _level(name, 1)
    g, Rc = load_npz(SC.FILE_PRED(name, 1)), trees['Rc']
    xd, rd = x.to(DEV), r.to(DEV)
    at = lambda p: (p[:, SC.PRED_FRAMES(ori[0]), :5, ::SC.PRED_ROWS].double().cpu().numpy(), p[:, :, 5, 0, 0].double().cpu().numpy())
    good04, good5 = at(Rc.reconstruct(xd, shape, ori, rd, upsample_type='space', half=40))
    off04, off5 = at(Rc.reconstruct(xd, shape, ori, rd, upsample_type=None, half=40))
    half04, half5 = at(Rc.reconstruct(xd, shape, ori, rd, upsample_type='space', half=20))
    dflt04, dflt5 = at(Rc.reconstruct(xd, shape, ori, rd, upsample_type='space'))
    r04, r5 = g['pred04'].astype(np.float64), g['pred5'].astype(np.float64)
    assert _relmax(good04, r04) < 1e-5 and _relmax(good5, r5) < 1e-5
    assert _relmax(off04, r04) > 1e-2 and np.array_equal(off5, good5)                        # the offset moves the block, not the smoke-out rows
    assert _relmax(half5, r5) > 1e-2 and np.array_equal(half04, good04) and np.array_equal(dflt5, half5)


def test_reconstruct_level_batch_invariance(trees):
    Rc = trees['Rc']
    x, r, shape, ori, half, up, _ = _level('small', 1)
    xd, rd = x.to(DEV), r.to(DEV)
    both = Rc.reconstruct(xd, shape, ori, rd, upsample_type=up, half=half)
    for b in range(2):
        assert torch.equal(Rc.reconstruct(xd[b:b + 1], shape, ori, rd, upsample_type=up, half=half), both[b:b + 1])
    wide = torch.randn(2, 26, 82, 80, 88, device=DEV)
    view = wide[:, 1:25, :, :, :80]
    view.copy_(xd)
    assert not view.is_contiguous() and torch.equal(Rc.reconstruct(view, shape, ori, rd, upsample_type=up, half=half), both)


# ----------------------------------------------------------------------------------------------------- scoring
@pytest.mark.parametrize('level', [0, 1])
def test_score_super_four_comparisons(trees, level):
    Sc = trees['Sc']
    g, pred, data = load_npz(SC.FILE_SCORE), SC.score_pred(level).to(DEV), SC.score_data().to(DEV)
    r = Sc.score_super(pred, data, W_E)
    m = SC.metrics_super_fp64(pred.cpu().numpy(), data.cpu().numpy(), W_E)
    assert Sc.COMPARISONS == ('base', 'current', 'linear', 'nearest')
    for k in Sc.KEYS:
        assert r[k].dtype == np.float64 and r[k].shape == (4, SC.SCORE_B) == m[k].shape
        err = float(np.abs(r[k] - m[k]).max() / np.abs(m[k]).max())
        print(f'  level {level} {k}: per-sample rel {err:.2e}')
        assert err <= 1e-10, (k, err)                                                       # fp64 sums of at most 4 * 3 * 128 * 128 terms, reordered
    for k, mk in REF_KEYS:
        for i, cmp in enumerate(Sc.COMPARISONS):
            exact, ref = float(m[mk][i].mean()), float(g[f'level{level}::{k}'][i])
            hip_err, ref_err = abs(r[mk][i].mean() - exact) / abs(exact), abs(ref - exact) / abs(exact)
            print(f'level {level} {cmp} {k}: hip {hip_err:.2e} reference {ref_err:.2e} from the fp64 evaluation')
            assert A.gate(hip_err, ref_err, factor=1.0, slack=1e-12), (k, cmp, hip_err, ref_err)
    # base and current are score() on the strided views
    n, N = pred.shape[-1], data.shape[-1]
    sp, f = n // (N // 2), N // n
    base = Sc.score(pred[:, :, :, ::sp, ::sp], [data[:, :, c, ::2, ::2] for c in range(6)], W_E)
    cur = Sc.score(pred, [data[:, :, c, ::f, ::f] for c in range(6)], W_E)
    for k in Sc.KEYS:
        assert np.allclose(r[k][0], base[k], rtol=1e-12, atol=0) and np.allclose(r[k][1], cur[k], rtol=1e-12, atol=0), k
    one = Sc.score_super(pred[1:], data[1:], W_E)
    for k in r:
        assert one[k].tobytes() == r[k][:, 1:].tobytes(), k                                  # a sample's result does not depend on the batch
    view = torch.randn(SC.SCORE_B, SC.SCORE_T, 7, N, N + 8, device=DEV)[:, :, :6, :, :N]     # the data as a view with wider rows
    view.copy_(data)
    two = Sc.score_super(pred, view, W_E)
    for k in r:
        assert two[k].tobytes() == r[k].tobytes(), k


# ----------------------------------------------------------------------------------------------------- the driver
def _args(**over):
    kw = dict(is_wavelet=True, is_condition_control=True, image_size=64, device=DEV, upsample=1, is_super_model=True, w_energy=W_E, w_init=0.4,
              wave_type='bior1.3', pad_mode='zero')
    kw.update(over)
    return types.SimpleNamespace(**kw)


def test_multi_evaluate_super_returns_the_reference_arrays(trees, tmp_path):
    g = load_npz(SC.FILE_SCORE)
    ppl = trees['INF'].InferencePipeline([object(), object()], {}, SC.rescaler(), results_path=str(tmp_path), args_general=_args())
    for level in range(2):
        pred, data = SC.score_pred(level).to(DEV), SC.score_data()
        out = ppl.multi_evaluate(pred, data, plot=False)
        assert torch.equal(pred[:, 0, 0].cpu(), data[:, 0, 0, ::2 - level, ::2 - level])      # the initial condition is written into pred
        assert len(out) == 5
        for (k, _), arr in zip(REF_KEYS, out):
            ref = g[f'level{level}::{k}'].astype(np.float64)
            assert arr.shape == (4,) and np.all(np.abs(arr - ref) <= 1e-5 * np.abs(ref)), (level, k, arr, ref)


def test_end_to_end_cascade(trees, tmp_path):
    """Two tiny real models (dim 8, 3 ancestral steps) at the reference's tensor sizes, guided by CascadeGuidance: run_model returns two
    preds that equal the chain sample -> super_conditions -> sample_with_source -> reconstruct bit for bit under the same noise, both levels
    take the fused guided step, and run() writes results_sim.txt with two blocks of four entries. dim_mults is (1, 2, 4), the depth of the
    full-size models: with (1, 2) the super model's middle attention would run over 40 x 40 = 1600 tokens of the 80 x 80 tensor, and the
    attention kernels take at most 1024 (csrc/attention.hip: attn_fwd_choose), so that model cannot be built here at this tensor size."""
    name = 'small'
    c = SC.CASES[name]
    shape, ori = [list(s) for s in c['shape']], [list(o) for o in c['ori']]
    resc = SC.rescaler().to(DEV)
    torch.manual_seed(5)
    kw = dict(loss_layer_weight=None, is_condition_control=True, is_condition_pad=True, is_wavelet=True, wave_type='bior1.3', pad_mode='zero',
              image_size=40, frames=24, timesteps=3, standard_fixed_ratio=0.05, coeff_ratio=0.3)
    m0 = trees['GD'](trees['Unet3D'](dim=8, dim_mults=(1, 2, 4), channels=42, resnet_groups=4), is_super_model=False, padded_shape=shape[0],
                     ori_shape=ori[0], **kw).to(DEV)
    m1 = trees['GD'](trees['Unet3D'](dim=8, dim_mults=(1, 2, 4), channels=82, resnet_groups=4), is_super_model=True, padded_shape=shape,
                     ori_shape=ori, **kw).to(DEV)
    gk = dict(is_condition_control=True, w_energy=W_E, w_init=0.4)
    fn = trees['Gd'].CascadeGuidance([trees['Gd'].SmokeGuidance(shape[0], ori[0], resc[:, :, 40:], **gk), trees['Gd'].SmokeGuidance(shape[1], ori[1], resc, **gk)])
    assert fn.fused_step and all(g.fused_step for g in fn.levels)
    guided = []
    for lvl, g in enumerate(fn.levels):
        g.guide = (lambda lvl, inner: lambda *a, **k: guided.append(lvl) or inner(*a, **k))(lvl, g.guide)
    args = _args()
    ppl = trees['INF'].InferencePipeline([m0, m1], {'design_fn': fn, 'design_guidance': 'standard'}, resc, results_path=str(tmp_path / 'out'), args_general=args)
    state = SC.fine_state(name)

    def seed():
        gen = torch.Generator(device=DEV).manual_seed(23)
        for m in (m0, m1):
            m.sample_noise = lambda shp, device: torch.randn(tuple(shp), device=device, generator=gen)
    seed()
    preds = ppl.run_model(state)
    assert len(preds) == 2 and [tuple(p.shape) for p in preds] == [(2, 16, 6, 32, 32), (2, 16, 6, 64, 64)]
    assert all(bool(torch.isfinite(p).all()) for p in preds)
    assert 0 in guided and 1 in guided                                                       # both levels went through the fused guided step
    # the stage-by-stage chain under the same noise
    seed()
    base = state.to(DEV)[:, :, :, ::2, ::2].contiguous()
    from ddpm.data_2d import pack_smoke_fields
    packed = pack_smoke_fields(base[:, :, :5].permute(0, 2, 1, 3, 4).contiguous(), torch.zeros(2, 16, device=DEV), resc.reshape(-1)[-42:], pad_t=24, pad_x=40)
    skw = dict(batch_size=2, design_fn=fn, design_guidance='standard')
    out0 = m0.sample(low=None, init=packed[:, :, -2].contiguous(), init_u=base[:, 0, 0], control=packed[:, :, 24:40].contiguous(), **skw)
    src = trees['Cs'].super_conditions(out0, shape[0], state.to(DEV), resc, shape[1], 24, 80)
    low, init1, control1 = trees['Cs'].views(src)
    out1 = m1.sample_with_source(src, N_upsample=1, low=low, init=init1, init_u=state.to(DEV)[:, 0, 0], control=control1, **skw)
    assert tuple(out0.shape) == (2, 24, 42, 40, 40) and tuple(out1.shape) == (2, 24, 82, 80, 80)
    Rc = trees['Rc']
    assert torch.equal(preds[0], Rc.reconstruct(out0, shape[0], ori[0], Rc.level_rescaler(resc, 42), half=20))
    assert torch.equal(preds[1], Rc.reconstruct(out1, shape[1], ori[1], resc, upsample_type='space', half=40))
    assert torch.equal(out1[:, :, 40:80], low) and torch.equal(out1[:, :, -2], init1)        # the sampler re-imposes the conditions
    # the assembled source is what three copies into a zeroed tensor give
    seed()
    m0.sample(low=None, init=packed[:, :, -2].contiguous(), init_u=base[:, 0, 0], control=packed[:, :, 24:40].contiguous(), **skw)
    plain = m1.sample(N_upsample=1, low=low.contiguous(), init=init1.contiguous(), init_u=state.to(DEV)[:, 0, 0], control=control1.contiguous(), **skw)
    assert torch.equal(plain, out1)
    # run() on a one-batch list
    seed()
    ppl.run([(state, shape, ori, 0)])
    text = open(tmp_path / 'out' / 'results_sim.txt').read().split('\n')
    assert text[1] == str(args) and text[2] == 'Number of upsampling times: 0' and text[8] == 'Number of upsampling times: 1', text
    for blk in (text[3:8], text[9:14]):
        assert [line.split(':')[0] for line in blk] == ['J_total', 'J_target', 'J_energy', 'mse', 'n_l2']
        for line in blk:
            vals = [float(v) for v in line.split('[')[1].split(']')[0].split()]
            assert len(vals) == 4 and all(np.isfinite(vals)), line
    assert text[14].startswith('-----') and not os.path.exists(tmp_path / 'out' / 'results.txt')
