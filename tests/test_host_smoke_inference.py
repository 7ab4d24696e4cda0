"""Host-side checks of the smoke inference driver (wdno_amd/smoke/inference_2d.py, reconstruct.py: plan, score.py) against what the
reference's own run recorded (tests/golden/ref_smoke_inference*.npz and its manifest). No GPU and no built library needed."""
import inspect
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import smoke_inference_inputs as SI
from tests.helpers import GOLDEN, load_npz

with open(os.path.join(GOLDEN, 'ref_smoke_inference_manifest.json')) as _f:
    MAN = json.load(_f)


@pytest.fixture(scope='module')
def trees():
    from wdno_amd import tree_path
    for t in ('third_party', 'smoke'):
        p = tree_path(t)
        if p not in sys.path:
            sys.path.insert(0, p)
    import inference_2d as INF
    from wdno_amd.smoke import reconstruct as Rc, score as Sc
    return dict(INF=INF, Rc=Rc, Sc=Sc)


def test_drop_in_resolves_to_this_tree_and_binds_the_reference_call_sites(trees):
    """Every public callable takes the reference's parameters, by the names and in the order the reference's run recorded."""
    INF = trees['INF']
    assert os.path.abspath(INF.__file__).startswith(os.path.abspath(os.path.join(os.path.dirname(__file__), '..', 'wdno_amd', 'smoke')))
    assert len(MAN['signatures']) == 13
    for name, params in MAN['signatures'].items():
        obj = INF
        for part in name.split('.'):
            obj = getattr(obj, part)
        assert list(inspect.signature(obj).parameters) == params, name
    # the reference's call sites (inference_2d.py:466-479, 257, 272)
    inspect.signature(INF.InferencePipeline.__init__).bind(None, [None], {}, 1, results_path='x', args_general=None)
    inspect.signature(INF.InferencePipeline.multi_evaluate).bind(None, None, None, plot=False)
    inspect.signature(INF.guidance_fn).bind(None, None, None, None, None, w_energy=0, w_init=0, low=None, init=None, init_u=None)
    opts = {a.dest: a.default for a in INF.build_parser()._actions}
    assert opts['batch_size'] == 50 and opts['is_wavelet'] is False and opts['wave_type'] == 'bior1.3' and opts['w_init_list'] == [0]
    assert INF.build_parser().parse_args(['--is_wavelet', 'True', '--is_condition_control', 'True']).is_wavelet is True


def _args(**over):
    kw = dict(is_wavelet=True, is_condition_control=True, image_size=64, device='cpu', upsample=0, is_super_model=False, w_energy=0.0, w_init=0.0,
              wave_type='bior1.3', pad_mode='zero')
    kw.update(over)
    return types.SimpleNamespace(**kw)


def test_unsupported_configurations_name_the_reference_line(trees, tmp_path):
    INF = trees['INF']
    P = INF.InferencePipeline
    for over in (dict(is_wavelet=False), dict(is_super_model=True)):
        with pytest.raises(NotImplementedError, match=r'inference_2d\.py:\d+'):
            P([object()], {}, 1, results_path=str(tmp_path / 'r'), args_general=_args(**over))
    with pytest.raises(NotImplementedError, match=r'inference_2d\.py:155-232'):
        P([object(), object()], {}, 1, results_path=str(tmp_path / 'r'), args_general=_args())
    ppl = P([object()], {}, 1, results_path=str(tmp_path / 'r'), args_general=_args())
    assert os.path.isdir(tmp_path / 'r')
    with pytest.raises(NotImplementedError, match=r'inference_2d\.py:155-232'):
        ppl.run_super_model(None, None, None, None)
    for fn in (ppl.multi_evaluate, ppl.multi_evaluate_control):
        with pytest.raises(NotImplementedError, match=r'inference_2d\.py:372-378'):
            fn(torch.zeros(1, 2, 6, 4, 4), torch.zeros(1, 2, 6, 4, 4), plot=True)
    for over in (dict(is_wavelet=False), dict(is_super_model=True)):
        with pytest.raises(NotImplementedError, match=r'inference_2d\.py'):
            INF.load_model(_args(**over), (3, 6, 6), (2, 8, 8), torch.ones(1, 1, 42, 1, 1))
    with pytest.raises(NotImplementedError):
        INF.guidance_fn(torch.zeros(1), _args(is_wavelet=False), None, None, None)


def test_save_results_writes_the_reference_lines(trees, tmp_path):
    P = trees['INF'].InferencePipeline
    one = lambda v: {0: [np.array([v]), np.array([v + 2.0])]}
    for cc, fname in ((True, 'results_sim.txt'), (False, 'results.txt')):
        a = _args(is_condition_control=cc)
        P([object()], {}, 1, results_path=str(tmp_path), args_general=a).save_results(one(1.0), one(2.0), one(3.0), one(4.0), one(5.0))
        lines = open(tmp_path / fname).read().split('\n')
        assert lines[1] == str(a) and lines[2] == 'Number of upsampling times: 0'
        assert lines[3:8] == ['J_total: [2.],', 'J_target: [3.],', 'J_energy: [4.],', 'mse: [5.],', 'n_l2: [6.]'] and lines[8].startswith('-----')


def test_reconstruct_plan_integers_and_refusals(trees):
    """plan() refuses what the C side refuses (csrc/smoke_reconstruct.hip: validate)."""
    Rc = trees['Rc']
    p = Rc.plan((50, 24, 42, 40, 40), (18, 34, 34), (32, 64, 64))
    assert (p['tn'], p['hn'], p['lds_bytes'], p['half'], p['L'], p['mode']) == (4, 8, 21760, 20, 6, 1)
    assert (p['sample_stride'], p['frame_stride'], p['chan_stride'], p['row_stride']) == (24 * 42 * 1600, 42 * 1600, 1600, 40)
    q = Rc.plan((1, 8, 42, 12, 16), (6, 9, 11), (8, 14, 18))
    KH = q['hn'] // 2 + 2
    assert q['half'] == 6 and q['lds_bytes'] == 4 * (4 * q['tn'] * KH * 11 + 2 * q['tn'] * q['hn'] * 11) <= 65536
    assert Rc.plan((1, 4, 42, 8, 8), (3, 3, 3), (2, 2, 2))['lds_bytes'] >= 8 * 256          # the smoke-out workgroup's reduction tree
    v = Rc.plan((2, 12, 42, 40, 40), (10, 18, 18), (16, 32, 32), strides=(2 * 12 * 84 * 1600, 84 * 1600, 1600, 40, 1))
    assert v['frame_stride'] == 84 * 1600
    xs, shape, ori = (3, 6, 42, 16, 16), (5, 12, 12), (6, 20, 20)
    for wave, mode in (('bior2.4', 'periodization'), ('bior1.3', 'periodization'), ('bior2.4', 'zero')):
        with pytest.raises(ValueError):
            Rc.plan(xs, shape, ori, wave, mode)
    for bad_ori in ((8, 20, 20), (6, 21, 20), (6, 20, 22), (0, 20, 20)):               # a crop larger than the (6, 20, 20) reconstruction
        with pytest.raises(ValueError):
            Rc.plan(xs, shape, bad_ori)
    for bad_shape in ((7, 12, 12), (5, 17, 12), (5, 12, 17), (2, 12, 12)):              # a block larger than the tensor / shorter than the filter
        with pytest.raises(ValueError):
            Rc.plan(xs, bad_shape, (1, 1, 1))
    with pytest.raises(ValueError):
        Rc.plan((3, 6, 41, 16, 16), shape, ori)
    for bad in ((6 * 42 * 256, 42 * 256, 256, 16, 2), (6 * 42 * 256, 42 * 256, 256, 8, 1), (6 * 42 * 256, 256, 42 * 256, 16, 1)):
        with pytest.raises(ValueError):
            Rc.plan(xs, shape, ori, strides=bad)                                          # strided columns, overlapping rows, channel-major frames
    with pytest.raises(ValueError):
        Rc.plan((1, 6, 42, 16, 4200), (5, 12, 4100), (6, 20, 8196))                       # the smallest tile would not fit the LDS budget


def test_score_refuses_tensors_it_cannot_describe(trees):
    Sc = trees['Sc']
    with pytest.raises(RuntimeError):
        Sc.score(torch.zeros(1, 2, 6, 4, 4), [torch.zeros(1, 2, 4, 4)] * 6, 0.0)         # pred on the CPU: no fallback
    assert Sc.KEYS == ('mse', 'mse_wo_smoke', 'n_l2', 'J_target', 'J_energy', 'J_total')


@pytest.mark.parametrize('name', sorted(SI.CASES))
def test_numpy_fp64_metrics_reproduce_the_reference_run(name):
    """The arbiter of the GPU score tests: multi_evaluate's formulas in plain numpy fp64 on the regenerated inputs give the five arrays the
    reference's own multi_evaluate returned -- to fp64 rounding in control mode (the reference scores an fp64 solver_out), to fp32 rounding in
    simulation mode (the reference computes in fp32 there: 1e-5 covers fp32 sums of 1e6 terms)."""
    g, c = load_npz(SI.FILE_OF[name]), MAN['cases'][name]
    pred = SI.score_pred(name).numpy()
    if c['is_condition_control']:
        s = 128 // pred.shape[-1]
        data, tol = SI.score_data_sim(name).numpy()[:, :, :, ::s, ::s], 1e-5
        assert c['metric_dtype'] == 'float32'
    else:
        data, tol = SI.score_data_control(name), 1e-12
        assert c['metric_dtype'] == 'float64'
    m = SI.metrics_fp64(pred, data, MAN['w_energy'])
    for k in ('J_total', 'J_target', 'J_energy', 'mse', 'n_l2'):
        ref = float(g[f'{name}::{k}'][0])
        assert abs(m[k].mean() - ref) <= tol * abs(ref), (name, k, m[k].mean(), ref)


@pytest.mark.parametrize('name', sorted(SI.CASES))
def test_oracle_rebuild_of_the_exact_pred_equals_the_reference_fp64_run(name):
    """The exact pred of the GPU gate is rebuilt with oracle/dwt_ref.py; at the stored entries it equals the reference's own fp64 run."""
    g, (tshape, shape, ori, _, _) = load_npz(SI.FILE_OF[name]), SI.CASES[name]
    e = SI.exact_pred(*SI.sample_output(name), shape, ori, 20)
    want04 = g[f'{name}::pred04'].astype(np.float64) - g[f'{name}::diff04']
    want5 = g[f'{name}::pred5'].astype(np.float64) - g[f'{name}::diff5']
    assert np.abs(e[:, SI.PRED_FRAMES(ori[0]), :5, ::SI.PRED_ROWS] - want04).max() < 1e-12
    assert np.abs(e[:, :, 5, 0, 0] - want5).max() < 1e-12 and np.abs(e[:, :, 5] - e[:, :, 5, :1, :1]).max() == 0.0
    r = g[f'{name}::ref_err']
    assert abs(np.abs(e[:, :, :5]).max() - r[1]) < 1e-12 and abs(np.abs(e[:, :, 5]).max() - r[3]) < 1e-12
    assert 0 < r[0] / r[1] < 1e-6 and 0 < r[2] / r[3] < 1e-6                              # the reference's own fp32 error


def test_main_reaches_run_without_forking(trees, tmp_path, monkeypatch):
    """main(args): load_data -> load_model (SmokeGuidance as design_fn on the loader's diffusion) -> inference -> InferencePipeline.run, and
    nothing on that way forks. The data and checkpoint loaders (the reference's ddpm.utils, which need files) and run() itself are doubles."""
    INF = trees['INF']
    from wdno_amd.smoke.guidance import SmokeGuidance
    resc, loader, dif, seen = torch.ones(1, 1, 42, 1, 1), [('state', 'shape', 'ori_shape', 0)], object(), {}
    fake = types.ModuleType('ddpm.utils')
    fake.load_data = lambda a: (loader, [18, 34, 34], [32, 64, 64], resc)
    fake.load_ddpm_base_model = lambda a, shape, ori, r: seen.update(loaded=(shape, ori)) or (dif, 'cpu')
    monkeypatch.setitem(sys.modules, 'ddpm.utils', fake)
    monkeypatch.setattr(os, 'fork', lambda: (_ for _ in ()).throw(AssertionError('forked')))
    monkeypatch.setattr(INF.InferencePipeline, 'run', lambda self, dl: seen.update(run=(self, dl)))
    args = INF.build_parser().parse_args(['--is_wavelet', 'True', '--w_energy', '0.7', '--inference_result_path', str(tmp_path)])
    args.device, args.standard_fixed_ratio, args.coeff_ratio, args.w_init = 'cpu', 0.05, 0.0, 1.3
    args.inference_result_subpath = str(tmp_path / 'sub')
    INF.main(args)
    ppl, dl = seen['run']
    assert dl is loader and ppl.model == [dif] and seen['loaded'] == ([18, 34, 34], [32, 64, 64]) and os.path.isdir(tmp_path / 'sub')
    fn = ppl.args['design_fn']
    assert isinstance(fn, SmokeGuidance) and fn.fused_step and ppl.args['design_guidance'] == 'standard'
    assert (fn.shape, fn.ori_shape, fn.is_condition_control, fn.w_energy, fn.w_init) == ((18, 34, 34), (32, 64, 64), False, 0.7, 1.3)
