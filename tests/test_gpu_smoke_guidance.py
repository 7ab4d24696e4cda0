"""The smoke control-objective guidance on the GPU: csrc/smoke_guidance.hip through wdno_amd/smoke/guidance.py (SmokeGuidance) and the fused
guided step of diffusion_core.sampling_loop, against the reference's own gradients (tests/golden/ref_guidance.npz), the existing closed form
(guidance_fn_explicit), fp64 finite differences of the restated objective (oracle/guidance_ref.py) and the existing guided routes. GPU box only.

Shapes, as tensor / coefficient block / field crop -- the smallest at which tiling, cropping and padding can each go wrong:
  (i)   [2, 4, 42, 8, 8]    / (3, 6, 6)    / (2, 8, 8)     the tiny model's state; half = H // 2
  (ii)  [3, 6, 42, 16, 16]  / (5, 12, 12)  / (6, 20, 20)   block smaller than the tensor on every axis; several tiles
  (iii) [2, 24, 42, 40, 40] / (18, 34, 34) / (32, 64, 64)  full size: the cases `full` and `full_control` of the fixture
  (iv)  [1, 6, 82, 16, 16]  / as (ii)                      C != 42: smoke-out at channel 81
  (v)   [2, 4, 42, 8, 8]    / (4, 6, 6)    / (3, 7, 5)     crop smaller than the (4, 8, 8) reconstruction on every axis, odd sizes
A bior1.3 / zero axis of v coefficients reconstructs 2 v - 4 samples, so a block of 5 frames gives 6: the crop of (ii) and (iv) has 6 frames
(with 8, guidance_fn_explicit's slices clamp silently but its helper _success_gradient(5, 8) indexes frame 7 of a 6-frame synthesis, and the
kernel is to refuse such a crop), and (v) carries the crop-smaller-than-the-reconstruction case.

Gates: rel-L2 < 1e-5 between two fp32 evaluations of the same expression; identical bits wherever the same launches run twice (batch
independence, graph replay against eager) and wherever g is structurally zero; tests/arbiter.gate for the chains."""
import sys

import numpy as np
import pytest
import torch

from tests import arbiter as A
from tests.helpers import load_npz, manifest, rel_l2, weights

pytestmark = pytest.mark.gpu
DEV = 'cuda'
M = manifest()

SHAPES = {
    'i': ((2, 4, 42, 8, 8), (3, 6, 6), (2, 8, 8)),
    'ii': ((3, 6, 42, 16, 16), (5, 12, 12), (6, 20, 20)),
    'iii': ((2, 24, 42, 40, 40), (18, 34, 34), (32, 64, 64)),
    'iv': ((1, 6, 82, 16, 16), (5, 12, 12), (6, 20, 20)),
    'v': ((2, 4, 42, 8, 8), (4, 6, 6), (3, 7, 5)),
}
W_E, W_I = 0.7, 1.3


@pytest.fixture(scope='module')
def trees():
    from wdno_amd import tree_path
    for t in ('third_party', 'smoke', 'burgers'):
        p = tree_path(t)
        if p not in sys.path:
            sys.path.insert(0, p)
    from video_diffusion_pytorch.video_diffusion_pytorch_conv3d import Unet3D_with_Conv3D
    from ddpm.diffusion_2d import GaussianDiffusion as GD2
    from wdno_amd.smoke import guidance as Gd
    from wdno_amd import diffusion_core as K
    return dict(Unet3D=Unet3D_with_Conv3D, GD2=GD2, Gd=Gd, K=K)


def _inputs(name, seed, B=None, scale=0.4):
    """x [B, F, C, H, W] (dense: the kernel must ignore what lies outside the block), RESCALER, init_u on the GPU."""
    tshape, shape, ori = SHAPES[name]
    tshape = tshape if B is None else (B,) + tshape[1:]
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(tshape, device=DEV, generator=gen) * scale
    init_u = torch.randn(tshape[0], ori[1], ori[2], device=DEV, generator=gen)
    resc = torch.linspace(1.0, 5.0, tshape[2], device=DEV).reshape(1, 1, -1, 1, 1)
    return x, resc, init_u, shape, ori


def _structure_mask(x, shape):
    tc, hc, wc = shape
    m = torch.zeros_like(x, dtype=torch.bool)
    m[:, :tc, :40, :hc, :wc] = True
    m[:, :tc, -1] = True
    return m


# ----------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize('name', ['full', 'full_control', 'small_b2', 'small_no_weights'])
def test_gradient_vs_reference_run(trees, name):
    """Gradient mode against the gradients the reference's own guidance_fn returned: the gate of
    tests/test_gpu_data.py::test_smoke_guidance_gradient_vs_reference_run, and exactly zero outside the block and the smoke-out channel."""
    from tests.test_oracle_dwt import guidance_case
    x, resc, init_u, g_ref, kw = guidance_case(name)
    shape, ori = kw.pop('shape'), kw.pop('ori_shape')
    fn = trees['Gd'].SmokeGuidance(shape, ori, resc.to(DEV), **kw)
    assert fn.graph_safe and fn.fused_step
    g = fn(x.to(DEV), low=None, init=None, init_u=init_u.to(DEV))
    e = rel_l2(g, g_ref)
    print(f'{name}: SmokeGuidance vs the reference run {e:.3e}')
    assert g.shape == x.shape and g.dtype == torch.float32
    assert e < 1e-5, (name, e)
    assert float(g[~_structure_mask(g, shape)].abs().max()) == 0.0


# ----------------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize('with_u', [True, False])
@pytest.mark.parametrize('cc', [False, True])
@pytest.mark.parametrize('name', ['i', 'ii', 'iv', 'v'])
def test_gradient_vs_closed_form(trees, name, cc, with_u):
    Gd = trees['Gd']
    x, resc, init_u, shape, ori = _inputs(name, 3)
    u = init_u if with_u else None
    kw = dict(is_condition_control=cc, w_energy=W_E, w_init=W_I)
    g = Gd.SmokeGuidance(shape, ori, resc, **kw)(x, init_u=u)
    ref = Gd.guidance_fn_explicit(x, shape, ori, resc, init_u=u, **kw)
    assert torch.equal(g == 0, ref == 0), (name, cc, with_u, int(((g == 0) != (ref == 0)).sum()))
    if cc and not with_u:
        assert float(g.abs().max()) == 0.0
        return
    e = rel_l2(g, ref)
    print(f'({name}) cc={cc} init_u={with_u}: kernel vs guidance_fn_explicit {e:.3e}')
    assert e < 1e-5, (name, cc, with_u, e)


def test_gradient_vs_finite_differences_full_size(trees):
    """Shape (iii): three directional derivatives of the fp64 restatement of J (oracle/guidance_ref.py), the tolerance of
    tests/test_gpu_data.py::test_smoke_guidance_gradient_vs_oracle_finite_difference."""
    from oracle import guidance_ref as G
    rng = np.random.default_rng(9)
    shape, ori = SHAPES['iii'][1:]
    x = np.zeros((1, 24, 42, 40, 40))
    x[:, :18, :, :34, :34] = rng.standard_normal((1, 18, 42, 34, 34)) * 0.3
    x[:, :18, -1] = rng.standard_normal((1, 18, 40, 40)) * 0.3
    resc = np.linspace(1.0, 9.0, 42).reshape(1, 1, 42, 1, 1)
    init_u = rng.standard_normal((1, 64, 64))
    fn = trees['Gd'].SmokeGuidance(shape, ori, torch.from_numpy(resc).float().to(DEV), w_energy=W_E, w_init=W_I)
    g = fn(torch.from_numpy(x).float().to(DEV), init_u=torch.from_numpy(init_u).float().to(DEV)).double().cpu().numpy()
    xs = x * resc
    for seed in range(3):
        v = np.random.default_rng(100 + seed).standard_normal(xs.shape)
        fd = G.directional_derivative(xs, v, shape, ori, init_u, W_E, W_I)
        print(f'direction {seed}: <g, v> = {(g * v).sum():.9e}, central difference {fd:.9e}')
        assert abs((g * v).sum() - fd) < 2e-5 * max(1.0, abs(fd)), (seed, (g * v).sum(), fd)


# ----------------------------------------------------------------------------------------------------- C
class _Sched(torch.nn.Module):
    def __init__(self, K, T=1000):
        super().__init__()
        K.register_schedule(self, K.cosine_beta_schedule(T), lambda snr: torch.ones_like(snr))
        self.num_timesteps = T


@pytest.mark.parametrize('clip', [False, True])
@pytest.mark.parametrize('name', ['ii', 'iii'])
def test_fused_mode_equals_the_torch_composition(trees, name, clip):
    """eps' = eps + g(x0) s[t] with x0 = c1[t] x_t - c2[t] eps (clamped when clip) and one t per sample."""
    Gd, K = trees['Gd'], trees['K']
    x_t, resc, init_u, shape, ori = _inputs(name, 21)
    B = x_t.shape[0]
    eps = torch.randn(x_t.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(22))
    t = torch.tensor([999, 400, 0], device=DEV, dtype=torch.long).repeat(B)[:B]
    mod = _Sched(K).to(DEV)
    fn = Gd.SmokeGuidance(shape, ori, resc, w_energy=W_E, w_init=W_I).set_init_u(init_u)
    ex = lambda a: a[t].reshape(B, 1, 1, 1, 1)
    x0 = ex(mod.sqrt_recip_alphas_cumprod) * x_t - ex(mod.sqrt_recipm1_alphas_cumprod) * eps
    if clip:
        x0 = x0.clamp(-1., 1.)
    grad = Gd.guidance_fn_explicit(x0, shape, ori, resc, w_energy=W_E, w_init=W_I, init_u=init_u)
    # the schedule entry of every sample puts its guidance term at the size of eps (rms 1) where g is not zero: a term far below eps would
    # be lost to the rounding of the sum in either evaluation
    nz = grad != 0
    s_table = torch.zeros(1000, device=DEV)
    s_table[t] = 1.0 / (grad.flatten(1).pow(2).sum(1) / nz.flatten(1).sum(1)).sqrt()
    term_ref = grad * ex(s_table)
    out = fn.guide(mod, x_t, eps, t, s_table, clip)
    assert torch.equal(out[~nz], eps[~nz])                               # bit for bit wherever g = 0
    term = (out - eps)[nz]
    size = float(term_ref[nz].pow(2).mean().sqrt())
    e = rel_l2(term, term_ref[nz])
    print(f'({name}) fused guidance term (clip={clip}): rms {size:.3f} against eps rms 1; vs torch composition {e:.3e}')
    assert 0.1 < size < 10.0
    assert e < 1e-5, e
    assert torch.equal(fn.guide(mod, x_t, eps, t, torch.zeros(1000, device=DEV), clip), eps)


# ----------------------------------------------------------------------------------------------------- D
def test_batch_independence_and_determinism(trees):
    Gd, K = trees['Gd'], trees['K']
    x_t, resc, init_u, shape, ori = _inputs('ii', 31, B=5)
    gen = torch.Generator(device=DEV).manual_seed(32)
    eps = torch.randn(x_t.shape, device=DEV, generator=gen)
    t = torch.randint(0, 1000, (5,), device=DEV, generator=gen)
    s_table = torch.rand(1000, device=DEV, generator=gen)
    mod = _Sched(K).to(DEV)
    fn = Gd.SmokeGuidance(shape, ori, resc, w_energy=W_E, w_init=W_I).set_init_u(init_u)
    grad, fused = fn(x_t, init_u=init_u), fn.guide(mod, x_t, eps, t, s_table, True)
    assert torch.equal(grad, fn(x_t, init_u=init_u)) and torch.equal(fused, fn.guide(mod, x_t, eps, t, s_table, True))
    assert float(grad.abs().max()) > 0 and not torch.equal(fused, eps)
    for b in (0, 2, 4):
        one = Gd.SmokeGuidance(shape, ori, resc, w_energy=W_E, w_init=W_I).set_init_u(init_u[b:b + 1])
        assert torch.equal(one(x_t[b:b + 1], init_u=init_u[b:b + 1]), grad[b:b + 1]), b
        assert torch.equal(one.guide(mod, x_t[b:b + 1], eps[b:b + 1], t[b:b + 1], s_table, True), fused[b:b + 1]), b


# ----------------------------------------------------------------------------------------------------- E, F: chains on the tiny smoke model
def _smoke(trees, **over):
    gz = load_npz('ref_smoke_diffusion.npz')
    c = M['smoke_diffusion']
    u, d = c['unet'], dict(c['diffusion'])
    d['padded_shape'] = tuple(d['padded_shape']); d['ori_shape'] = tuple(d['ori_shape'])
    d.update(over)
    net = trees['Unet3D'](dim=u['dim'], dim_mults=tuple(u['dim_mults']), channels=u['channels'], resnet_groups=u['resnet_groups'])
    dif = trees['GD2'](net, loss_layer_weight=torch.from_numpy(gz['lw']), **d)
    dif.load_state_dict({k: v for k, v in weights(gz, 'w::').items() if k.startswith('model.')}, strict=False)
    return gz, dif.to(DEV)


def _run(dif, use_graph, seed, **kw):
    g = torch.Generator(device=DEV).manual_seed(seed)
    dif.sample_noise = lambda shape, device: torch.randn(tuple(shape), device=device, generator=g)
    dif.use_graph = use_graph
    out = dif.sample(**kw)
    torch.cuda.synchronize()
    return out


CHAINS = {'ddim10': (dict(timesteps=1000, sampling_timesteps=10, ddim_sampling_eta=1.0), 'standard'),
          'ddpm12': (dict(timesteps=12, sampling_timesteps=None), 'standard-alpha')}


@pytest.fixture(scope='module')
def chain_setup(trees):
    torch.manual_seed(1)
    shape, ori = SHAPES['i'][1:]
    resc = torch.linspace(1.0, 5.0, 42).reshape(1, 1, 42, 1, 1).to(DEV)
    gz = load_npz('ref_smoke_diffusion.npz')
    return dict(shape=shape, ori=ori, resc=resc, init=torch.from_numpy(gz['ddim_init']).to(DEV), u1=torch.randn(2, 8, 8, device=DEV),
                u2=torch.randn(2, 8, 8, device=DEV) * 3.0)


def _dif(trees, chain):
    over, mode = CHAINS[chain]
    _, dif = _smoke(trees, is_condition_control=False, **over)
    dif.standard_fixed_ratio = 0.05
    return dif, mode


@pytest.mark.parametrize('chain', sorted(CHAINS))
def test_guided_chain_replay_equals_eager_and_stays_close(trees, chain_setup, chain):
    """(a) graph replay = eager, bit for bit; (b) the new route is no further from the GuidanceFn route than 1.5 x the distance between the
    GuidanceFn route and the reference-style autograd callback (+ 1e-6): two fp32 evaluations of the same chain the project already trusts."""
    Gd, c = trees['Gd'], chain_setup
    dif, mode = _dif(trees, chain)
    kw = dict(batch_size=2, design_guidance=mode, init=c['init'], init_u=c['u1'])
    new_fn = Gd.SmokeGuidance(c['shape'], c['ori'], c['resc'], w_energy=W_E, w_init=W_I)
    new = _run(dif, True, 41, design_fn=new_fn, **kw)
    assert len(trees['K']._graph_cache.get(dif, {})) == 1
    eager = _run(dif, False, 41, design_fn=new_fn, **kw)
    assert torch.isfinite(new).all() and torch.equal(new, eager)
    old = _run(dif, False, 41, design_fn=Gd.GuidanceFn(c['shape'], c['ori'], c['resc'], w_energy=W_E, w_init=W_I), **kw)
    auto = lambda xx, low=None, init=None, init_u=None: Gd.guidance_fn(xx, c['shape'], c['ori'], c['resc'], init_u=init_u, w_energy=W_E, w_init=W_I)
    ref = _run(dif, False, 41, design_fn=auto, **kw)
    plain = _run(dif, False, 41, batch_size=2, init=c['init'])
    d_new, d_ref, d_plain = rel_l2(new, old), rel_l2(old, ref), rel_l2(new, plain)
    print(f'{chain}: SmokeGuidance vs GuidanceFn {d_new:.3e}; GuidanceFn vs autograd callback {d_ref:.3e}; SmokeGuidance vs unguided {d_plain:.3e}')
    assert A.gate(d_new, d_ref), (d_new, d_ref)
    assert d_plain > 1e-3                      # the guidance is not a no-op on this chain


def test_set_init_u_replays_the_captured_graph(trees, chain_setup):
    """(c) a second sample() with a new init_u replays the same graph on the new density, never on the first call's tensor;
    (d) the fixed ratio reaches the replayed step."""
    Gd, K, c = trees['Gd'], trees['K'], chain_setup
    dif, mode = _dif(trees, 'ddim10')
    fn = Gd.SmokeGuidance(c['shape'], c['ori'], c['resc'], w_energy=W_E, w_init=40.0)
    u1 = c['u1'].clone()
    kw = dict(batch_size=2, design_fn=fn, design_guidance=mode)
    g1 = _run(dif, True, 51, init=c['init'], init_u=u1, **kw)
    graphs = dict(K._graph_cache[dif])
    u1.fill_(float('nan'))
    g2 = _run(dif, True, 51, init=c['init'] * 0.5, init_u=c['u2'], **kw)
    after = K._graph_cache[dif]
    assert len(after) == len(graphs) == 1 and all(after[k] is v for k, v in graphs.items())
    e2 = _run(dif, False, 51, init=c['init'] * 0.5, init_u=c['u2'], **kw)
    assert torch.isfinite(g2).all() and torch.equal(g2, e2) and not torch.equal(g1, g2)
    dif.standard_fixed_ratio = 0.02
    g3 = _run(dif, True, 51, init=c['init'] * 0.5, init_u=c['u2'], **kw)
    e3 = _run(dif, False, 51, init=c['init'] * 0.5, init_u=c['u2'], **kw)
    assert torch.equal(g3, e3) and not torch.equal(g3, g2)


def test_workspace_of_a_captured_step_survives_other_batch_sizes(trees, chain_setup):
    """(c') one object, batch 2 captured, then a batch-3 sample() and a full-size gradient call (both need a larger workspace), then batch 2
    again: the batch-2 graph is replayed (still cached: the cache keeps two graphs) on the workspace it captured, which is still the
    object's, and equals eager."""
    Gd, K, c = trees['Gd'], trees['K'], chain_setup
    dif, mode = _dif(trees, 'ddim10')
    fn = Gd.SmokeGuidance(c['shape'], c['ori'], c['resc'], w_energy=W_E, w_init=W_I)
    kw = dict(design_fn=fn, design_guidance=mode)
    g2 = _run(dif, True, 71, batch_size=2, init=c['init'], init_u=c['u1'], **kw)
    sg2 = next(iter(K._graph_cache[dif].values()))
    ws2 = {k: (v, v.data_ptr()) for k, v in fn._ws.items()}
    assert len(ws2) == 1
    init3, u3 = torch.cat((c['init'], c['init'][:1] * 0.7)), torch.cat((c['u1'], c['u2'][:1]))
    g3 = _run(dif, True, 71, batch_size=3, init=init3, init_u=u3, **kw)
    big = torch.randn(4, 4, 42, 8, 8, device=DEV) * 0.3
    fn(big, init_u=torch.randn(4, 8, 8, device=DEV))
    assert len(fn._ws) == 3 and all(fn._ws[k] is v and v.data_ptr() == p for k, (v, p) in ws2.items())      # kept, not replaced
    assert any(v is sg2 for v in K._graph_cache[dif].values())
    r2 = _run(dif, True, 71, batch_size=2, init=c['init'], init_u=c['u1'], **kw)
    assert any(v is sg2 for v in K._graph_cache[dif].values()) and len(K._graph_cache[dif]) == 2
    e2 = _run(dif, False, 71, batch_size=2, init=c['init'], init_u=c['u1'], **kw)
    e3 = _run(dif, False, 71, batch_size=3, init=init3, init_u=u3, **kw)
    assert torch.equal(r2, g2) and torch.equal(r2, e2) and torch.equal(g3, e3) and torch.isfinite(g3).all()


def test_guide_refuses_mismatched_operands(trees):
    Gd, K = trees['Gd'], trees['K']
    x_t, resc, init_u, shape, ori = _inputs('i', 5)
    eps, mod = torch.randn_like(x_t), _Sched(K).to(DEV)
    t, s = torch.zeros(2, device=DEV, dtype=torch.long), torch.zeros(1000, device=DEV)
    fn = Gd.SmokeGuidance(shape, ori, resc, w_energy=W_E, w_init=W_I).set_init_u(init_u)
    assert torch.equal(fn.guide(mod, x_t, eps, t, s, True), eps)
    for bad in (dict(x_t=x_t[:1]), dict(t=t.int()), dict(t=t[:1]), dict(s=torch.zeros(2000, device=DEV)), dict(s=s.double())):
        a = {**dict(x_t=x_t, t=t, s=s), **bad}
        with pytest.raises(ValueError):
            fn.guide(mod, a['x_t'], eps, a['t'], a['s'], True)


def test_other_routes_are_unchanged(trees, chain_setup, monkeypatch):
    """F: GuidanceFn still runs guided_sampling_loop_smoke, a plain autograd callable still runs the eager loop, and neither reaches the
    guidance kernel or the fused loop."""
    Gd, K, c = trees['Gd'], trees['K'], chain_setup
    dif, mode = _dif(trees, 'ddim10')
    kw = dict(batch_size=2, design_guidance=mode, init=c['init'], init_u=c['u1'])
    old_fn = Gd.GuidanceFn(c['shape'], c['ori'], c['resc'], w_energy=W_E, w_init=W_I)
    auto = lambda xx, low=None, init=None, init_u=None: Gd.guidance_fn(xx, c['shape'], c['ori'], c['resc'], init_u=init_u, w_energy=W_E, w_init=W_I)
    calls = []
    smoke_loop, loop = K.guided_sampling_loop_smoke, K.sampling_loop
    monkeypatch.setattr(K, 'guided_sampling_loop_smoke', lambda *a, **k: calls.append('smoke') or smoke_loop(*a, **k))
    monkeypatch.setattr(K, 'sampling_loop', lambda *a, **k: calls.append('fused') or loop(*a, **k))
    monkeypatch.setattr(Gd.SmokeGuidance, '_launch', lambda *a, **k: (_ for _ in ()).throw(AssertionError('the guidance kernel was launched')))
    a = _run(dif, True, 61, design_fn=old_fn, **kw)
    assert calls == ['smoke']
    b = _run(dif, False, 61, design_fn=old_fn, **kw)
    assert torch.equal(a, b) and calls == ['smoke', 'smoke']
    ref = _run(dif, True, 61, design_fn=auto, **kw)
    assert calls == ['smoke', 'smoke']                           # the eager loop: neither of the two graph loops
    assert rel_l2(a, ref) < 1e-4                                 # (the bar tests/test_gpu_graph.py holds these two routes to)
    # the same bits as the loops give when called the way the parent commit's dispatch calls them
    desc = dif._desc(tuple(a.shape), dif._coef_shape(tuple(a.shape), 0))
    src = dif._condition_source(tuple(a.shape), DEV, c['init'], None, None)
    g = torch.Generator(device=DEV).manual_seed(61)
    dif.sample_noise = lambda shape, device: torch.randn(tuple(shape), device=device, generator=g)
    x = K.apply_cond(dif.sample_noise(tuple(a.shape), DEV).contiguous(), src, desc)
    direct = smoke_loop(dif, x, src, desc, old_fn, mode, ddim_pairs=K.ddim_time_pairs(dif.num_timesteps, dif.sampling_timesteps),
                        eta=dif.ddim_sampling_eta, low=None, init=c['init'], init_u=c['u1'], use_graph=True)
    assert torch.equal(direct, a)
