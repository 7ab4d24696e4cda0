"""Host-side checks of the Burgers control-objective guidance (wdno_amd/burgers/guidance.py, diffusion_core.guided_sampling_loop_burgers):
the closed-form gradient against the reference's autograd result and central differences, the schedule table, the sampler's dispatch and
the launch plan. No GPU and no built library needed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import burgers_guidance_inputs as GI, burgers_guidance_ref as GR
from tests.helpers import GOLDEN

G = np.load(os.path.join(GOLDEN, 'ref_burgers_guidance.npz'))
with open(os.path.join(GOLDEN, 'ref_burgers_guidance_manifest.json')) as f:
    META = json.load(f)


@pytest.fixture(scope='module')
def trees():
    from wdno_amd import tree_path
    for t in ('third_party', 'burgers'):
        p = tree_path(t)
        if p not in sys.path:
            sys.path.insert(0, p)
    from ddpm_burgers import model_utils as MU
    from ddpm_burgers.diffusion_1d import GaussianDiffusion
    return dict(MU=MU, GD=GaussianDiffusion)


def test_manifest_matches_the_input_module():
    assert set(META['cases']) == set(GI.CASES)
    for name, c in GI.CASES.items():
        assert META['cases'][name] == {k: (list(v) if isinstance(v, tuple) else v) for k, v in c.items()}


@pytest.mark.parametrize('name', sorted(GI.CASES))
def test_closed_form_equals_reference_autograd_and_central_differences(name):
    """The formula the kernel implements (include/wdno_hip.h) in fp64 numpy: 1e-10 relative from the gradient the reference's autograd
    returned in fp64, exactly zero outside the coefficient block, and 1e-8 from central differences of J."""
    c = GI.CASES[name]
    x, resc, ut = (v.double().numpy() for v in GI.case_input(name))
    h, w = c['shape']
    kw = dict(shape=c['shape'], ori=c['ori'], wu=c['wu'], wf=c['wf'], condition_f=c['condition_f'])
    g = GR.gradient(x, resc, ut, **kw)
    ref = G[f'{name}::g64']
    err = np.linalg.norm(g[:, :8, :h, :w] - ref) / np.linalg.norm(ref)
    rest = g.copy()
    rest[:, :8, :h, :w] = 0
    print(name, 'closed form vs reference fp64', err)
    assert err < 1e-10 and np.abs(rest).max() == 0.0 and float(G[f'{name}::rest64']) == 0.0
    # central differences along random directions inside the block and along single entries: J is quadratic, so they are exact up to rounding
    rng = np.random.default_rng(GI.seed_of(name))
    scale = np.abs(g).max()
    for trial in range(6):
        d = np.zeros_like(x)
        if trial < 3:
            d[:, :8, :h, :w] = rng.standard_normal((x.shape[0], 8, h, w))
        else:
            d[tuple(rng.integers(0, s) for s in (x.shape[0], 8, h, w))] = 1.0
        d /= np.linalg.norm(d)
        e = 1e-3
        fd = (GR.value(x + e * d, resc, ut, **kw) - GR.value(x - e * d, resc, ut, **kw)) / (2 * e)
        an = float((g * d).sum())
        assert abs(fd - an) <= 1e-8 * max(abs(an), scale), (name, trial, fd, an)


@pytest.mark.parametrize('sched', [None, 'cosine', 'sigmoid', 'sigmoid_flip'])
def test_s_table_is_the_schedule_rounded_to_fp32(trees, sched):
    from wdno_amd import diffusion_core as K
    fn = trees['MU'].get_scheduler(sched)
    tab = K.guidance_s_table(fn, 1000)
    assert tab.dtype == torch.float32 and tab.device.type == 'cpu' and tuple(tab.shape) == (1000,)
    for t in range(1000):
        want = np.float32(1.0) if fn is None else np.float32(float(fn(t)))
        assert tab[t].item() == want, (sched, t)
    # a python-float schedule (the constant ones the evaluation scripts pass as lambdas)
    assert torch.equal(K.guidance_s_table(lambda t: 0.2, 6), torch.full((6,), 0.2, dtype=torch.float64).float())


class _Net(torch.nn.Module):
    channels, self_condition = 9, False

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))


@pytest.mark.parametrize('ddim', [False, True])
def test_dispatch_selects_the_fused_loop_only_for_graph_safe_guidance(trees, ddim, monkeypatch):
    """Which sample() keyword combinations take guided_sampling_loop_burgers (the loops are mocked; nothing is launched)."""
    from wdno_amd import diffusion_core as K

    class Fused:
        graph_safe = True

        def guide(self, *a):
            raise AssertionError('mocked')

        def __call__(self, x):
            raise AssertionError('mocked')

    class SafeWithoutStep:               # capturable launches, but no fused step of its own
        graph_safe = True

        def __call__(self, x):
            raise AssertionError('mocked')

    def plain(x):
        raise AssertionError('mocked')
    calls = []
    monkeypatch.setattr(K, 'guided_sampling_loop_burgers', lambda mod, x, src, desc, guidance, s_table, **kw: calls.append(('fused', guidance, s_table, kw)) or x)
    monkeypatch.setattr(K, 'sampling_loop', lambda mod, x, *a, **kw: calls.append(('unguided',)) or x)
    monkeypatch.setattr(K, 'apply_cond', lambda x, src, desc: x)

    def build(objective='pred_noise'):
        dif = trees['GD'](_Net(), seq_length=(16, 16), padded_shape=[11, 14], ori_shape=[20, 28], pad_mode='periodization', wave_type='bior2.4',
                          timesteps=1000, sampling_timesteps=4 if ddim else None, objective=objective, is_condition_u0=True)
        # the general (eager) form ends in model_predictions: make reaching it observable instead of running a network
        dif.model_predictions = lambda *a, **k: (_ for _ in ()).throw(LookupError('general form'))
        dif.sample_noise = lambda shape, device: torch.zeros(tuple(shape))
        return dif

    def route(dif, **kw):
        calls.clear()
        try:
            dif.sample(batch_size=2, u_init=torch.zeros(2, 8, 16), **kw)
        except LookupError:
            return 'general'
        assert len(calls) == 1
        return calls[0][0]
    fused, dif = Fused(), build()
    assert route(dif) == 'unguided'
    assert route(dif, nablaJ=fused) == 'fused'
    assert calls[0][1] is fused and torch.equal(calls[0][2], torch.ones(1000)) and calls[0][3].get('use_graph') is None
    assert ('ddim_pairs' in calls[0][3]) == ddim
    sched = trees['MU'].get_scheduler('cosine')
    assert route(dif, nablaJ=fused, J_scheduler=sched) == 'fused' and torch.equal(calls[0][2], K.guidance_s_table(sched, 1000))
    assert route(dif, nablaJ=plain) == 'general'                                              # a plain callable: today's path
    assert route(dif, nablaJ=trees['MU'].get_nablaJ(lambda x: x.sum())) == 'general'
    assert route(dif, nablaJ=SafeWithoutStep()) == 'general'
    assert route(dif, nablaJ=fused, proj_guidance=lambda ep, nj: ep + nj) == 'general'        # batch-wide projections stay eager
    assert route(dif, nablaJ=fused, pred_noise=torch.zeros(2, 9, 16, 16)) == 'general'
    for objective in ('pred_x0', 'pred_v'):
        assert route(build(objective), nablaJ=fused) == 'general'
    dif.self_condition = True
    with pytest.raises((LookupError, AssertionError)):
        calls.clear()
        dif.sample(batch_size=2, u_init=torch.zeros(2, 8, 16), nablaJ=fused)
    assert not calls


def test_plan_pins_the_descriptor_integers():
    from wdno_amd.burgers import guidance as BG
    base = BG.plan((50, 9, 64, 64), (41, 60), (81, 120))
    assert base == dict(B=50, C=9, H=64, W=64, sample_stride=9 * 4096, chan_stride=4096, row_stride=64, h=41, w=60, n_t=81, n_x=120, L=10, mode=0,
                        ntile=4, tw=15, lds_bytes=4 * (20 + 4 * 41 * 23 + 2 * 80 * 23 + 80 * 38), u_rows=[0, 1, 2, 38, 39, 40])
    assert base['lds_bytes'] == 42048 and base['lds_bytes'] <= BG.LDS_BUDGET
    assert BG.plan((50, 9, 64, 64), (41, 60), (81, 120), condition_f=True)['u_rows'] == [0, 1, 2, 39, 40]
    # the super-resolution model: 17 channels, the first eight read, coefficient block of padded_shape[k - 1]
    sup = BG.plan((2, 17, 32, 32), (21, 28), (41, 56), is_super_model=True)
    assert sup == dict(B=2, C=17, H=32, W=32, sample_stride=17 * 1024, chan_stride=1024, row_stride=32, h=21, w=28, n_t=41, n_x=56, L=10, mode=0,
                       ntile=2, tw=14, lds_bytes=4 * (20 + 4 * 21 * 22 + 2 * 40 * 22 + 40 * 36), u_rows=[0, 1, 2, 18, 19, 20])
    big = BG.plan((2, 17, 128, 128), (82, 120), (161, 240), is_super_model=True)              # tall blocks get narrower tiles
    assert (big['tw'], big['ntile']) == (10, 12) and big['lds_bytes'] <= BG.LDS_BUDGET
    # u_rows covers the coefficient rows whose gradient the closed form leaves non-zero (bior2.4 has zero taps inside its 10: row 2 is reached
    # by tap 0 only, which is 0 in both synthesis filters)
    c = GI.CASES['small']
    x, resc, ut = (v.double().numpy() for v in GI.case_input('small'))
    g = GR.gradient(x, resc, ut, c['shape'], c['ori'], 1.0, 0.0)
    nonzero = [k for k in range(c['shape'][0]) if np.abs(g[:, :4, k]).max() > 0]
    assert BG.u_rows(c['shape'][0], c['ori'][0], 10) == [0, 1, 2, 6, 7, 8] and nonzero == [0, 1, 6, 7, 8]
    for bad in (dict(wave_type='db4'), dict(pad_mode='zero'), dict(wave_type='bior1.3', pad_mode='zero')):
        with pytest.raises(ValueError):
            BG.plan((2, 9, 64, 64), (41, 60), (81, 120), **bad)
    with pytest.raises(ValueError):
        BG.plan((2, 9, 2048, 64), (2000, 60), (3999, 120))                                     # a one-column tile would not fit the LDS budget
    for shape, ori, xs in (((41, 60), (81, 120), (2, 7, 64, 64)), ((41, 70), (81, 120), (2, 9, 64, 64)), ((41, 60), (83, 120), (2, 9, 64, 64)),
                           ((4, 60), (8, 120), (2, 9, 64, 64))):
        with pytest.raises(ValueError):
            BG.plan(xs, shape, ori)


def test_plan_needs_no_library_or_gpu(tmp_path):
    """plan() in a process where the shared library cannot be found and no device is visible."""
    code = ('import os, sys\n'
            'import wdno_amd._lib as L\n'
            f'L.LIB_PATH = {str(tmp_path / "missing.so")!r}\n'
            'from wdno_amd.burgers import guidance as BG\n'
            'p = BG.plan((50, 9, 64, 64), (41, 60), (81, 120))\n'
            'assert (p["ntile"], p["tw"]) == (4, 15)\n'
            'assert L._lib is None\n'
            'print("ok")\n')
    env = dict(os.environ, HIP_VISIBLE_DEVICES='', CUDA_VISIBLE_DEVICES='')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, '-c', code], cwd=root, env=env, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == 'ok', r.stdout + r.stderr


def test_guidance_object_falls_back_for_other_wavelets():
    """A (wave, mode) the kernel is not built for: the object is still a nablaJ, but not graph_safe (the sampler keeps the autograd path)."""
    from wdno_amd.burgers import guidance as BG
    ut = torch.zeros(2, 20, 28)
    assert BG.BurgersGuidance((11, 14), (20, 28), GI.RESCALER, ut, 1.0, 0.1).graph_safe is True
    assert BG.BurgersGuidance((11, 14), (20, 28), GI.RESCALER, ut, 1.0, 0.1, wave_type='db4').graph_safe is False
    g = BG.get_nablaJ_2dconv(shape=[11, 14], ori_shape=[20, 28], RESCALER=torch.tensor(GI.RESCALER).view(1, 9, 1, 1), u_target=ut, wu=0.5, wf=0.05,
                             condition_f=True, target_i=0, device=0, dataset='1d', N_upsample=0, low=0)
    assert isinstance(g, BG.BurgersGuidance) and g.key() == ((11, 14), (20, 28), 0.5, 0.05, True, 'bior2.4', 'periodization', False)
    # set_target refills the same buffer
    buf = g.target
    g.set_target(torch.ones(2, 20, 28))
    assert g.target is buf and float(buf.min()) == 1.0 and tuple(buf.shape) == (2, 2, 28)
