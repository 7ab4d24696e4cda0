"""Host-side checks of the Burgers cascade (wdno_amd/burgers/cascade.py: plan and the CPU route of super_conditions;
super_shapes, load_super_model; eval_ddpm_burgers.py: the refusals) against what the reference's own evaluate recorded
(tests/golden/ref_burgers_cascade.npz and its manifest). No GPU and no built library needed."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import arbiter as A
from tests import burgers_cascade_inputs as CI, burgers_cascade_ref as CR
from tests.helpers import GOLDEN, load_npz
from wdno_amd.burgers import cascade as CS

with open(os.path.join(GOLDEN, 'ref_burgers_cascade_manifest.json')) as _f:
    MAN = json.load(_f)


@pytest.fixture(scope='module')
def trees():
    from wdno_amd import tree_path
    for t in ('third_party', 'burgers'):
        p = tree_path(t)
        if p not in sys.path:
            sys.path.insert(0, p)
    import eval_ddpm_burgers as E
    from ddpm_burgers import test_util as TU
    return dict(E=E, TU=TU)


@pytest.fixture(scope='module')
def gold():
    return load_npz('ref_burgers_cascade.npz')


_inputs = {}


def level_inputs(k):
    """(x_prev, the level's target view, RESCALER [1, 17, 1, 1]) of the hand-off into level k, as the reference's evaluate forms them; shared."""
    if k not in _inputs:
        h0, w0 = CI.SHAPES[k - 1]
        x_prev = (CI.sample_output(k - 1) * CI.rescaler(k - 1))[:, :8, :h0, :w0]
        step = 2 ** (CI.UPSAMPLE - k)
        _inputs[k] = (x_prev, CI.super_test_file()['u'][:, ::step, ::step], CI.rescaler(1))
    return _inputs[k]


# ------------------------------------------------------------------------------------------------ plan()
def test_plan_integers():
    pl = CS.plan((50, 8, 41, 60), (50, 161, 240), (81, 120), 128, 128)
    assert (pl['B'], pl['C'], pl['h0'], pl['w0'], pl['h1'], pl['w1'], pl['n_t'], pl['n_x'], pl['P_t'], pl['P_x']) == (50, 17, 41, 60, 81, 120, 161, 240, 128, 128)
    assert (pl['prev_sample_stride'], pl['prev_chan_stride'], pl['prev_row_stride']) == (8 * 41 * 60, 41 * 60, 60)
    assert (pl['tgt_sample_stride'], pl['tgt_row_stride'], pl['tgt_col_stride']) == (161 * 240, 240, 1)
    assert (pl['tile'], pl['ntile'], pl['grid'], pl['lds_bytes'], pl['L'], pl['mode'], pl['cond_u0'], pl['cond_uT']) == (16, 8, (8, 17, 50), 2048, 10, 0, 1, 1)
    # the second level, a strided block and a target read through row and column strides of 2; a ragged last tile
    pl = CS.plan((2, 8, 81, 120), (2, 321, 512), (161, 240), 256, 256, True, False, strides=(17 * 128 * 128, 128 * 128, 128, 1),
                 target_strides=(641 * 1024, 2048, 2))
    assert (pl['prev_row_stride'], pl['tgt_row_stride'], pl['tgt_col_stride'], pl['n_x'], pl['ntile'], pl['cond_uT']) == (128, 2048, 2, 480, 16, 0)
    pl = CS.plan((1, 8, 9, 13), (1, 33, 52), (17, 26), 20, 28)
    assert (pl['tile'], pl['ntile'], pl['grid'], pl['lds_bytes']) == (16, 2, (2, 17, 1), 16 * 28)


@pytest.mark.parametrize('kw', [
    dict(wave_type='bior1.3'), dict(pad_mode='zero'), dict(prev_shape=(2, 9, 9, 13)), dict(target_shape=(3, 33, 52)), dict(pad_t=18), dict(pad_x=30),
    dict(pad_x=4096), dict(shape1=(18, 26)), dict(shape1=(17, 27)), dict(pad_t=16), dict(pad_x=24), dict(target_shape=(2, 1, 52)),
    dict(target_shape=(2, 33, 51)), dict(prev_shape=(2, 8, 3, 2), shape1=(5, 4), target_shape=(2, 9, 8)), dict(strides=(8 * 9 * 13, 9 * 13, 12, 1)),
    dict(strides=(8 * 9 * 13, 9 * 13, 13, 2)), dict(strides=(7 * 9 * 13, 9 * 13, 13, 1)), dict(strides=(8 * 9 * 13, 8 * 13, 13, 1)),
    dict(target_strides=(33 * 52, 52, 0)), dict(target_strides=(33 * 52, -52, 1)), dict(prev_shape=(70000, 8, 9, 13), target_shape=(70000, 33, 52))])
def test_plan_refuses(kw):
    base = dict(prev_shape=(2, 8, 9, 13), target_shape=(2, 33, 52), shape1=(17, 26), pad_t=20, pad_x=28)
    base.update(kw)
    with pytest.raises(ValueError):
        CS.plan(**base)


# ------------------------------------------------------------------------------------------------ the fp64 evaluation and the CPU route
@pytest.mark.parametrize('k', [1, 2])
def test_cascade_ref_is_pinned_to_the_reference_fp64_run(gold, k):
    m = MAN['levels'][str(k)]
    x_prev, tgt, r = level_inputs(k)
    e = CR.condition(tgt, r, CI.SHAPES[k][1], m['P'], m['P'])
    assert np.abs(e[:, m['cond_rows'], :CI.SHAPES[k][1]] - gold[f'{k}::cond64_rows']).max() < 1e-12
    assert abs(np.abs(e).max() - m['cond_max']) < 1e-12 and float(np.abs(e[:, :, CI.SHAPES[k][1]:]).max()) == 0.0
    # the reference's fp32 channel is within its recorded error of it, and that error is fp32 rounding
    err = np.abs(gold[f'{k}::cond_rows'].astype(np.float64) - e[:, m['cond_rows'], :CI.SHAPES[k][1]]).max()
    assert abs(err - m['cond_err']) < 1e-12 and m['cond_err'] < 1e-6 * max(1.0, m['cond_max'])
    # low: the fp32 division, bit for bit
    low = CR.low32(x_prev, r)
    assert list(low.shape[2:]) == m['low_box'] and np.array_equal(low[:, :, ::CI.LOW_STEP[0], ::CI.LOW_STEP[1]], gold[f'{k}::low_sub'])
    assert float(low.astype(np.float64).sum()) == pytest.approx(m['low_sum'], rel=1e-12, abs=1e-9)


@pytest.mark.parametrize('k', [1, 2])
def test_cpu_route_against_the_reference_run(gold, k):
    m = MAN['levels'][str(k)]
    x_prev, tgt, r = level_inputs(k)
    P, (h1, w1) = m['P'], CI.SHAPES[k]
    assert not tgt.is_contiguous() or k == CI.UPSAMPLE
    src = CS.super_conditions(x_prev, tgt, r, (h1, w1), P, P)
    assert tuple(src.shape) == (CI.B, 17, P, P) and src.dtype == torch.float32 and src.is_contiguous()
    low, u_init, u_final = CS.views(src)
    assert low.data_ptr() == src[:, 8:16].data_ptr() and tuple(u_init.shape) == tuple(u_final.shape) == (CI.B, P // 2, P)
    bh, bw = m['low_box']
    assert np.array_equal(low[:, :, :bh:CI.LOW_STEP[0], :bw:CI.LOW_STEP[1]].numpy(), gold[f'{k}::low_sub'])
    assert float(low.double().sum()) == pytest.approx(m['low_sum'], rel=1e-12, abs=1e-9)
    assert float(low.double().abs().sum()) == pytest.approx(m['low_abs_sum'], rel=1e-12)          # nothing outside the box
    assert np.array_equal(low[:, :, :bh, :bw].numpy(), CR.low32(x_prev, r))
    cond = torch.cat((u_init, u_final), dim=1).double().numpy()
    e = CR.condition(tgt, r, w1, P, P)
    hip, ref = np.abs(cond - e).max() / np.abs(e).max(), m['cond_err'] / m['cond_max']
    print(f'level {k}: CPU route {hip:.3e} reference {ref:.3e}')
    assert A.gate(hip, ref, factor=1.5, slack=1e-6)
    assert float(src[:, :8].abs().max()) == 0.0 and float(np.abs(cond[:, :, w1:]).max()) == 0.0
    # one flag off: its stripes are zero, the others unchanged
    s0 = CS.super_conditions(x_prev, tgt, r, (h1, w1), P, P, True, False)
    assert torch.equal(s0[:, -1, :P // 2], src[:, -1, :P // 2]) and float(s0[:, -1, P // 2:].abs().max()) == 0.0 and torch.equal(s0[:, :16], src[:, :16])
    sT = CS.super_conditions(x_prev, tgt, r, (h1, w1), P, P, False, True)
    assert torch.equal(sT[:, -1, P // 2:], src[:, -1, P // 2:]) and float(sT[:, -1, :P // 2].abs().max()) == 0.0


def test_cpu_route_small_shapes_and_refusals():
    x, t, r = CI.small_case(3)
    src = CS.super_conditions(x, t, r, (17, 26), 20, 28)
    e = CR.conditions(x, t, r, (17, 26), 20, 28)
    assert np.array_equal(src[:, :16].numpy(), e[:, :16].astype(np.float32))
    assert np.abs(src[:, 16].double().numpy() - e[:, 16]).max() <= 1e-6 * np.abs(e[:, 16]).max()
    with pytest.raises(ValueError):
        CS.super_conditions(x, t, r[:16], (17, 26), 20, 28)
    with pytest.raises(ValueError):
        CS.super_conditions(x, t.double(), r, (17, 26), 20, 28)
    with pytest.raises(ValueError):
        CS.super_conditions(x, t, r, (19, 26), 20, 28)


@pytest.mark.parametrize('k', [0, 1, 2])
def test_fixture_fields_and_scores_are_consistent(gold, k):
    """What the fixture stores per level besides the hand-off: the fp64 fields of the level's sample (regenerated here from the hash inputs),
    the reference's fp32 error against them, and its five outputs in fp32 and fp64, which must be the same quantities."""
    from tests import burgers_eval_ref as ER
    m = MAN['levels'][str(k)]
    u, f = ER.reconstruct(CI.sample_output(k), CI.rescaler(k), CI.SHAPES[k], CI.ORI[k])
    assert u.shape == (CI.B, *CI.ORI[k]) and f.shape == (CI.B, CI.ORI[k][0] - 1, CI.ORI[k][1])
    assert np.abs(u[:, ::5, ::7] - gold[f'{k}::u64_sub']).max() < 1e-12 and np.abs(f[:, ::5, ::7] - gold[f'{k}::f64_sub']).max() < 1e-12
    assert abs(np.abs(u).max() - m['max_u']) < 1e-12 and abs(np.abs(f).max() - m['max_f']) < 1e-12
    assert m['err_u'] < 1e-6 * max(1.0, m['max_u']) and m['err_f'] < 1e-6 * max(1.0, m['max_f'])          # the reference's fields: fp32 rounding
    assert m['sub'] == 2 ** (CI.UPSAMPLE - k) and m['x_gt_shape'] == [CI.B, CI.ORI[k][0], CI.ORI[CI.UPSAMPLE][1]]
    for name in ('ddpm_mse', 'J_diffused', 'J_actual', 'energy', 'total_J'):
        v32, v64 = gold[f'{k}::{name}'], gold[f'{k}::{name}64']
        assert v32.dtype == np.float32 and v64.dtype == np.float64 and v32.shape == v64.shape
        assert np.abs(v32 - v64).max() <= 1e-5 * np.abs(v64).max(), (k, name)          # the bar of tests/test_host_burgers_eval.py for the same quantities: blocked fp32 sums against fp64
    # the level's energy divisor (test_util.py:96): sum f^2 / 4^k on the fp64 forcing, to the fp32 rounding of the recorded f
    assert np.abs(gold[f'{k}::energy64'] - np.square(f).sum((-1, -2)) / 4 ** k).max() <= 1e-5 * np.abs(gold[f'{k}::energy64']).max()
    assert np.abs(gold[f'{k}::total_J64'] - (gold[f'{k}::J_actual64'][0] + MAN['wf'] * gold[f'{k}::energy64'])).max() <= 1e-12 * np.abs(gold[f'{k}::total_J64']).max()


# ------------------------------------------------------------------------------------------------ the loader and the refusals
def test_super_model_shape_lists_and_channels(trees, monkeypatch):
    TU = trees['TU']
    from ddpm_burgers import train_diffusion as TD
    assert CS.super_shapes([41, 60], [81, 120], 3) == ([[81, 120], [161, 240], [321, 480]], [[161, 240], [321, 480], [641, 960]])
    made = {}

    class StubTrainer:
        def __init__(self, ddpm, dataset, **kw):
            made.update(ddpm=ddpm, dataset=dataset, kw=kw)

        def load(self, milestone):
            made['milestone'] = milestone
    stub = types.SimpleNamespace(shape=[41, 60], ori_shape=[81, 120])
    monkeypatch.setattr(TU, 'load_burgers_dataset_wavelet', lambda args, R: stub)
    monkeypatch.setattr(TD, 'Trainer', StubTrainer)
    args = trees['E'].build_parser().parse_args(['--exp_id', 'b', '--super_exp_id', 's', '--is_super_model', 'True', '--upsample_t', '2', '--upsample_x', '2',
                                                 '--is_condition_u0', 'True', '--is_condition_uT', 'True', '--using_ddim', 'True', '--ddim_sampling_steps', '4',
                                                 '--dim', '16', '--super_dim', '8', '--dim_muls', '1', '2', '--super_checkpoint', '7'])
    R = trees['E'].rescaler_table(args)
    assert R.flatten().tolist() == CI.RESCALER
    ddpm = trees['E'].load_2dconv_super_model('s', args, R)
    assert trees['E'].load_2dconv_super_model is CS.load_super_model
    assert ddpm.padded_shape == [[81, 120], [161, 240]] and ddpm.ori_shape == [[161, 240], [321, 480]]
    assert ddpm.channels == 17 and ddpm.is_super_model and tuple(ddpm.traj_size) == (256, 256) and ddpm.upsample_x == 2
    assert ddpm.model.init_conv.out_channels == 8 and args.dim == 16          # built with super_dim; args.dim put back for the next evaluate() of the loop
    assert made['kw']['is_super_model'] is True and made['milestone'] == 7 and made['kw']['results_folder'] == os.path.join('./results/', 's')


def test_out_of_scope_cases(trees):
    E, TU = trees['E'], trees['TU']
    args = types.SimpleNamespace(is_wavelet=True, is_super_model=False, wave_type='bior2.4', pad_mode='periodization', upsample_x=0, is_condition_f=False)
    ddpm = types.SimpleNamespace(is_wavelet=True, padded_shape=[41, 60], ori_shape=[81, 120], is_condition_f=False)
    sup = lambda **kw: types.SimpleNamespace(**{**vars(args), 'is_super_model': True, **kw})
    loaded = []
    real = E.load_2dconv_base_model
    E.load_2dconv_base_model = lambda *a, **k: loaded.append(a)
    try:
        cases = {
            '307': lambda: E.evaluate('m', 's', sup()),
            '175-178': lambda: E.diffuse_2dconv(ddpm, args, None, N_upsample=1, low=None),
            '207-218': lambda: E.diffuse_2dconv(ddpm, sup(is_condition_f=True), None),
            '207-218 ': lambda: E.evaluate('m', 's', sup(upsample_x=1, is_condition_f=True)),
            'test_util.py:236': lambda: E.load_2dconv_super_model('m', args, 1),
            '126-132': lambda: E.evaluate('m', 's', sup(upsample_x=1, is_wavelet=False)),
        }
        for line, fn in cases.items():
            with pytest.raises(NotImplementedError, match=r'reference burgers/.*' + line.strip()):
                fn()
    finally:
        E.load_2dconv_base_model = real
    assert not loaded                                # every refusal comes before anything is loaded
