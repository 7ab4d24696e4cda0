"""Host-side checks of the smoke control-objective guidance (wdno_amd/smoke/guidance.py: plan, SmokeGuidance; the dispatch and the schedule
table of smoke/ddpm/diffusion_2d.py). No GPU and no built library needed."""
import os
import subprocess
import sys

import pytest
import torch

# tensor / coefficient block / field crop of tests/test_gpu_smoke_guidance.py
SHAPES = {
    'i': ((2, 4, 42, 8, 8), (3, 6, 6), (2, 8, 8)),
    'ii': ((3, 6, 42, 16, 16), (5, 12, 12), (6, 20, 20)),
    'iii': ((2, 24, 42, 40, 40), (18, 34, 34), (32, 64, 64)),
    'iv': ((1, 6, 82, 16, 16), (5, 12, 12), (6, 20, 20)),
    'v': ((2, 4, 42, 8, 8), (4, 6, 6), (3, 7, 5)),
}


@pytest.fixture(scope='module')
def trees():
    from wdno_amd import tree_path
    for t in ('third_party', 'smoke'):
        p = tree_path(t)
        if p not in sys.path:
            sys.path.insert(0, p)
    from ddpm.diffusion_2d import GaussianDiffusion
    from wdno_amd.smoke import guidance as Gd
    return dict(GD=GaussianDiffusion, Gd=Gd)


@pytest.mark.parametrize('name', sorted(SHAPES))
def test_plan_integers(trees, name):
    Gd = trees['Gd']
    xs, shape, ori = SHAPES[name]
    B, F, C, H, W = xs
    (tc, hc, wc), (to, ho, wo) = shape, ori
    p = Gd.plan(xs, shape, ori)
    assert (p['B'], p['F'], p['C'], p['H'], p['W']) == xs and (p['tc'], p['hc'], p['wc']) == shape and (p['to'], p['ho'], p['wo']) == ori
    assert (p['sample_stride'], p['frame_stride'], p['chan_stride'], p['row_stride']) == (F * C * H * W, C * H * W, H * W, W)
    assert (p['L'], p['mode'], p['is_condition_control']) == (6, 1, 0)
    assert p['half'] == (20 if H > 20 else H // 2)
    assert p['ws_bytes'] == 4 * B * (2 * to * ho * wo + ho * wo)
    # the tiles: even synthesis tiles, LDS as the kernel lays it out and inside the budget, the grid covering crop and block
    tn, hn, kt, kh = p['tn'], p['hn'], p['kt'], p['kh']
    assert tn % 2 == 0 and hn % 2 == 0 and tn >= 2 and hn >= 2 and 1 <= kt <= tc and 1 <= kh <= hc
    KT, KH = tn // 2 + 2, hn // 2 + 2
    assert p['lds1_bytes'] == 4 * (2 * KT * KH * wc + 4 * KT * KH * wo + 2 * KT * hn * wo) <= Gd.LDS_BUDGET == 65536
    assert p['lds2_bytes'] == 4 * (2 * kt * (2 * kh + 4) * wo + 4 * kt * kh * wo) <= Gd.LDS_BUDGET
    assert -(-to // tn) * tn >= to and -(-ho // hn) * hn >= ho and -(-tc // kt) * kt >= tc and -(-hc // kh) * kh >= hc
    assert p['ncopy'] >= 1
    assert Gd.plan(xs, shape, ori, is_condition_control=True)['is_condition_control'] == 1


def test_plan_full_size_and_super_resolution_tiles(trees):
    Gd = trees['Gd']
    p = Gd.plan((50, 24, 42, 40, 40), (18, 34, 34), (32, 64, 64))
    assert (p['tn'], p['hn'], p['kt'], p['kh'], p['lds1_bytes'], p['lds2_bytes']) == (4, 8, 2, 4, 47488, 20480)
    assert p['ws_bytes'] == 50 * 1064960                       # 1.06 MB per sample
    q = Gd.plan((1, 24, 82, 80, 80), (18, 74, 74), (32, 144, 144))      # wide rows: smaller tiles
    assert (q['tn'], q['hn']) == (4, 4) and q['lds1_bytes'] <= Gd.LDS_BUDGET and q['half'] == 20


def test_plan_refuses_what_the_kernel_does_not_take(trees):
    Gd = trees['Gd']
    xs, shape, ori = SHAPES['ii']
    with pytest.raises(ValueError):
        Gd.plan(xs, shape, ori, 'bior2.4', 'periodization')
    with pytest.raises(ValueError):
        Gd.plan(xs, shape, ori, 'bior1.3', 'periodization')
    for bad_ori in ((8, 20, 20), (6, 21, 20), (6, 20, 22), (0, 20, 20)):          # a crop larger than the (6, 20, 20) reconstruction
        with pytest.raises(ValueError):
            Gd.plan(xs, shape, bad_ori)
    for bad_shape in ((7, 12, 12), (5, 17, 12), (5, 12, 17), (2, 12, 12)):         # a block larger than the tensor / shorter than the filter
        with pytest.raises(ValueError):
            Gd.plan(xs, bad_shape, (1, 1, 1))
    with pytest.raises(ValueError):
        Gd.plan((3, 6, 41, 16, 16), shape, ori)                                    # no room for 40 coefficient and 2 condition channels
    with pytest.raises(ValueError):
        Gd.plan((1, 6, 42, 16, 4200), (5, 12, 4100), (6, 20, 8196))                # the smallest tile would not fit the LDS budget


def test_plan_needs_no_library_or_gpu(tmp_path):
    code = ('import os, sys\n'
            'import wdno_amd._lib as L\n'
            f'L.LIB_PATH = {str(tmp_path / "missing.so")!r}\n'
            'from wdno_amd import tree_path\n'
            'sys.path[:0] = [tree_path("third_party"), tree_path("smoke")]\n'
            'from wdno_amd.smoke import guidance as Gd\n'
            'p = Gd.plan((2, 24, 42, 40, 40), (18, 34, 34), (32, 64, 64))\n'
            'assert (p["tn"], p["hn"]) == (4, 8)\n'
            'assert L._lib is None\n'
            'print("ok")\n')
    env = dict(os.environ, HIP_VISIBLE_DEVICES='', CUDA_VISIBLE_DEVICES='')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, '-c', code], cwd=root, env=env, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == 'ok', r.stdout + r.stderr


def test_guidance_object_flags_key_and_init_u_buffer(trees):
    Gd = trees['Gd']
    resc = torch.linspace(1.0, 5.0, 42).reshape(1, 1, 42, 1, 1)
    g = Gd.SmokeGuidance((3, 6, 6), (2, 8, 8), resc, w_energy=0.7, w_init=1.3)
    assert g.graph_safe is True and g.fused_step is True
    bad = Gd.SmokeGuidance((3, 6, 6), (2, 8, 8), resc, w_energy=0.7, w_init=1.3, wave_type='bior2.4', pad_mode='periodization')
    assert bad.graph_safe is False and bad.fused_step is False
    assert Gd.SmokeGuidance((3, 6, 6), (4, 8, 8), resc).fused_step is False          # a crop the reconstruction does not have
    assert Gd.GuidanceFn.graph_safe is True and not getattr(Gd.GuidanceFn, 'fused_step', False)
    assert g.key()[:7] == ((3, 6, 6), (2, 8, 8), False, 0.7, 1.3, 'bior1.3', 'zero') and g.key()[7] is None
    u = torch.ones(2, 8, 8)
    assert g.set_init_u(u) is g
    buf = g.init_u
    assert buf is not u and tuple(buf.shape) == (2, 8, 8) and g.key()[7] is not None
    k = g.key()
    u.fill_(float('nan'))
    g.set_init_u(torch.full((2, 8, 8), 2.0))
    assert g.init_u is buf and float(buf.min()) == 2.0 and g.key() == k              # refilled in place: a captured step reads the new density
    g.set_init_u(None)
    assert g.init_u is None and g.key()[7] is None
    g.set_init_u(torch.full((2, 8, 8), 3.0), device='cpu')
    assert g.init_u is buf and g.key() == k and float(buf.max()) == 3.0              # switched back on: the same buffer, the same key
    g.set_init_u(torch.zeros(3, 8, 8))
    assert g.init_u is not buf and tuple(g.init_u.shape) == (3, 8, 8)               # another batch size: a buffer of its own, the first one kept
    g.set_init_u(torch.ones(2, 8, 8))
    assert g.init_u is buf


class _Net(torch.nn.Module):
    channels, self_condition = 42, False

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))


def _dif(trees, ddim, **over):
    kw = dict(loss_layer_weight=None, is_condition_control=False, is_condition_pad=True, is_wavelet=True, is_super_model=False, wave_type='bior1.3',
              pad_mode='zero', padded_shape=(3, 6, 6), ori_shape=(2, 8, 8), image_size=8, frames=4, timesteps=1000,
              sampling_timesteps=10 if ddim else None, ddim_sampling_eta=1.0, standard_fixed_ratio=0.05, coeff_ratio=0.3)
    kw.update(over)
    return trees['GD'](_Net(), **kw)


@pytest.mark.parametrize('ddim', [False, True])
def test_s_table_equals_the_torch_expressions(trees, ddim):
    dif = _dif(trees, ddim)
    assert torch.equal(dif.guidance_s_table('standard'), torch.full((1000,), 0.05, dtype=torch.float32))
    want = (dif.coeff_ratio * dif.betas.flip(0)).float()
    tab = dif.guidance_s_table('standard-alpha')
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (1000,) and torch.equal(tab, want)
    # what model_predictions multiplies the gradient with at step t (diffusion_2d.py:733-741)
    t = torch.tensor([999, 400, 0])
    assert torch.equal(tab[t], (dif.coeff_ratio * dif.betas.clone().flip(0)).gather(-1, t))
    with pytest.raises(ValueError):
        dif.guidance_s_table('universal')


@pytest.mark.parametrize('ddim', [False, True])
def test_dispatch_selects_the_fused_loop_only_for_fused_step_objects(trees, ddim, monkeypatch):
    """Which design_fn takes sampling_loop with guidance (the loops are mocked; nothing is launched)."""
    from wdno_amd import diffusion_core as K

    class Fused:
        graph_safe = fused_step = True

        def __init__(self):
            self.u = 'unset'

        def set_init_u(self, u, device=None):
            self.u, self.device = u, device

        def key(self):
            return ()

        def __call__(self, x, **kw):
            raise AssertionError('mocked')

    class SafeOnly:                       # GuidanceFn's contract: capturable launches, no fused step
        graph_safe = True

        def __call__(self, x, **kw):
            raise AssertionError('mocked')

    def plain(x, **kw):
        raise AssertionError('mocked')
    calls = []
    monkeypatch.setattr(K, 'sampling_loop', lambda mod, x, src, desc, **kw: calls.append(('fused' if kw.get('guidance') is not None else 'unguided', kw)) or x)
    monkeypatch.setattr(K, 'guided_sampling_loop_smoke', lambda mod, x, src, desc, fn, mode, **kw: calls.append(('smoke', kw)) or x)
    monkeypatch.setattr(K, 'apply_cond', lambda x, src, desc: x)
    dif = _dif(trees, ddim)
    dif.model_predictions = lambda *a, **k: (_ for _ in ()).throw(LookupError('general form'))
    dif.sample_noise = lambda shape, device: torch.zeros(tuple(shape))
    init, u = torch.zeros(2, 4, 8, 8), torch.ones(2, 8, 8)

    def route(**kw):
        calls.clear()
        try:
            dif.sample(batch_size=2, init=init, init_u=u, **kw)
        except LookupError:
            return 'general'
        assert len(calls) == 1
        return calls[0][0]
    assert route() == 'unguided'
    fused = Fused()
    assert route(design_fn=fused, design_guidance='standard') == 'fused'
    kw = calls[0][1]
    assert kw['guidance'] is fused and fused.u is u and fused.device == torch.device('cpu') and kw['cond_first'] is False and ('ddim_pairs' in kw) == ddim
    assert torch.equal(kw['s_table'], dif.guidance_s_table('standard')) and kw['guidance_key'] == ('standard', 0.05, 0.3)
    assert route(design_fn=fused, design_guidance='standard-alpha') == 'fused'
    assert torch.equal(calls[0][1]['s_table'], dif.guidance_s_table('standard-alpha'))
    with pytest.raises(ValueError):
        route(design_fn=fused, design_guidance='universal')
    assert route(design_fn=SafeOnly()) == 'smoke'
    assert route(design_fn=trees['Gd'].GuidanceFn((3, 6, 6), (2, 8, 8), torch.ones(1, 1, 42, 1, 1))) == 'smoke'
    assert route(design_fn=plain) == 'general'
    unbuilt = trees['Gd'].SmokeGuidance((3, 6, 6), (2, 8, 8), torch.ones(1, 1, 42, 1, 1), wave_type='bior2.4', pad_mode='periodization')
    assert route(design_fn=unbuilt) == 'general'
    dif.self_condition = True
    assert route(design_fn=fused) == 'general'
