"""The Burgers control-objective guidance on the GPU: csrc/burgers_guidance.hip through wdno_amd/burgers/guidance.py and the graph-replayed
guided loop (diffusion_core.guided_sampling_loop_burgers), against the reference-generated fixtures of tests/golden/ref_burgers_guidance.npz
(tests/golden/make_ref_burgers_guidance_golden.py) and against the autograd route on the adjoint DWT kernels. GPU box only.

Gates: tests/arbiter.gate -- HIP no further from the fp64 value than 1.5 x the reference's own fp32 evaluation is (+ 1e-6) -- wherever a
fixture has the fp64 value; rel-L2 < 1e-5 (the north-star bar) between two fp32 evaluations of the same expression; identical bits wherever
the same launches run twice (batch independence, graph replay against eager, structural zeros)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import arbiter as A, burgers_guidance_inputs as GI
from tests.helpers import GOLDEN, rel_l2

pytestmark = pytest.mark.gpu
DEV = 'cuda'
G = np.load(os.path.join(GOLDEN, 'ref_burgers_guidance.npz'))
with open(os.path.join(GOLDEN, 'ref_burgers_guidance_manifest.json')) as f:
    META = json.load(f)
G2 = np.load(os.path.join(GOLDEN, 'ref_round2.npz'))


@pytest.fixture(scope='module')
def trees():
    from wdno_amd import tree_path
    for t in ('third_party', 'smoke', 'burgers'):
        p = tree_path(t)
        if p not in sys.path:
            sys.path.insert(0, p)
    from ddpm_burgers.unet import Unet2D
    from ddpm_burgers.diffusion_1d import GaussianDiffusion as GD1
    from ddpm_burgers import model_utils as MU
    from wdno_amd.burgers import guidance as BG
    from wdno_amd import diffusion_core as K
    return dict(Unet2D=Unet2D, GD1=GD1, MU=MU, BG=BG, K=K)


def _guidance(BG, name):
    c = GI.CASES[name]
    x, resc, ut = GI.case_input(name)
    g = BG.BurgersGuidance(c['shape'], c['ori'], resc, ut, c['wu'], c['wf'], condition_f=c['condition_f'], is_super_model=c['is_super'])
    return c, x.to(DEV), resc.to(DEV), ut.to(DEV), g


def _check_case(trees, name):
    c, x, resc, ut, g = _guidance(trees['BG'], name)
    h, w = c['shape']
    out = g(x)
    assert out.shape == x.shape and out.dtype == torch.float32
    exact, ref32 = G[f'{name}::g64'], G[f'{name}::g32']
    hip, ref = rel_l2(out[:, :8, :h, :w], exact), rel_l2(ref32, exact)
    rest = out.clone()
    rest[:, :8, :h, :w] = 0
    print(f'{name}: gradient vs fp64 -- hip {hip:.3e} reference fp32 {ref:.3e}; outside the block max |g| = {float(rest.abs().max())}')
    assert A.gate(hip, ref), (name, hip, ref)
    assert float(rest.abs().max()) == 0.0 and float(G[f'{name}::rest32']) == 0.0


@pytest.mark.parametrize('name', [n for n in sorted(GI.CASES) if not GI.CASES[n]['is_super']])
def test_gradient_vs_reference_fixture(trees, name):
    _check_case(trees, name)


def test_super_model_gradient_vs_reference_fixture(trees):
    """17 channels, x[:, :8] / RESCALER[:, :8] read, coefficient block of padded_shape[k - 1] (eval_ddpm_burgers.py:124, 327-332)."""
    _check_case(trees, 'super')


def _random_case(B, seed, condition_f=False, wu=0.7, wf=0.03):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(B, 9, 64, 64, device=DEV, generator=gen) * 0.4
    ut = torch.randn(B, 81, 120, device=DEV, generator=gen)
    resc = torch.tensor(GI.RESCALER, dtype=torch.float32, device=DEV).reshape(1, 9, 1, 1)
    return x, ut, resc, dict(shape=(41, 60), ori_shape=(81, 120), wu=wu, wf=wf, condition_f=condition_f)


@pytest.mark.parametrize('condition_f', [False, True])
def test_gradient_vs_autograd_on_the_adjoint_kernels_batch50(trees, condition_f):
    BG = trees['BG']
    x, ut, resc, kw = _random_case(50, 11, condition_f)
    g = BG.BurgersGuidance(kw['shape'], kw['ori_shape'], resc, ut, kw['wu'], kw['wf'], condition_f=condition_f)(x)
    with torch.enable_grad():
        xr = x.clone().requires_grad_(True)
        ref, = torch.autograd.grad(BG.guidance_value(xr, ut, kw['shape'], kw['ori_shape'], resc, kw['wu'], kw['wf'], condition_f), xr)
    e = rel_l2(g, ref)
    print('closed-form kernel vs autograd route, batch 50:', e)
    assert e < 1e-5, e


class _Sched(torch.nn.Module):
    def __init__(self, trees, T=1000):
        super().__init__()
        trees['K'].register_schedule(self, trees['K'].cosine_beta_schedule(T), lambda snr: torch.ones_like(snr))
        self.num_timesteps = T


@pytest.mark.parametrize('clip', [False, True])
def test_fused_mode_equals_the_torch_composition(trees, clip):
    """eps' = eps + nablaJ(x0) s[t] with x0 = c1[t] x_t - c2[t] eps (clamped when clip) and one t per sample."""
    BG = trees['BG']
    B = 6
    x_t, ut, resc, kw = _random_case(B, 21, wu=1.0, wf=0.05)
    gen = torch.Generator(device=DEV).manual_seed(22)
    eps = torch.randn(B, 9, 64, 64, device=DEV, generator=gen)
    t = torch.tensor([999, 700, 400, 150, 20, 0], device=DEV, dtype=torch.long)
    mod = _Sched(trees).to(DEV)
    g = BG.BurgersGuidance(kw['shape'], kw['ori_shape'], resc, ut, kw['wu'], kw['wf'])
    ex = lambda a: a[t].reshape(B, 1, 1, 1)
    x0 = ex(mod.sqrt_recip_alphas_cumprod) * x_t - ex(mod.sqrt_recipm1_alphas_cumprod) * eps
    if clip:
        x0 = x0.clamp(-1., 1.)
    grad = g(x0)
    # the schedule entry of every sample puts its guidance term at the size of eps (rms 1): a term far below eps would be lost to the rounding of
    # the sum in either evaluation
    s_table = torch.zeros(1000, device=DEV)
    s_table[t] = 1.0 / (grad.flatten(1).pow(2).sum(1) / (8 * 41 * 60)).sqrt()
    term_ref = grad * ex(s_table)
    out = g.guide(mod, x_t, eps, t, s_table, clip)
    h, w = kw['shape']
    mask = torch.zeros_like(eps, dtype=torch.bool)
    mask[:, :8, :h, :w] = True
    assert torch.equal(out[~mask], eps[~mask])                           # bit for bit wherever g = 0
    zero = (grad == 0) & mask                                            # (coefficient rows of field u beyond the filter's reach)
    assert torch.equal(out[zero], eps[zero])
    term = (out - eps)[mask]
    size = float(term_ref[mask].pow(2).mean().sqrt())
    e = rel_l2(term, term_ref[mask])
    print(f'fused guidance term (clip={clip}): rms {size:.3f} against eps rms 1; vs torch composition {e:.3e}; '
          f'eps\' identical to the composition: {torch.equal(out, eps + term_ref)}')
    assert 0.1 < size < 10.0
    assert e < 1e-5, e
    out0 = g.guide(mod, x_t, eps, t, torch.zeros(1000, device=DEV), clip)
    assert torch.equal(out0, eps)


def test_batch_independence_and_determinism(trees):
    BG = trees['BG']
    x_t, ut, resc, kw = _random_case(50, 31)
    gen = torch.Generator(device=DEV).manual_seed(32)
    eps = torch.randn(50, 9, 64, 64, device=DEV, generator=gen)
    t = torch.randint(0, 1000, (50,), device=DEV, generator=gen)
    s_table = torch.rand(1000, device=DEV, generator=gen)
    mod = _Sched(trees).to(DEV)
    g = BG.BurgersGuidance(kw['shape'], kw['ori_shape'], resc, ut, kw['wu'], kw['wf'])
    grad, fused = g(x_t), g.guide(mod, x_t, eps, t, s_table, True)
    assert torch.equal(grad, g(x_t)) and torch.equal(fused, g.guide(mod, x_t, eps, t, s_table, True))
    for b in (0, 17, 49):
        one = BG.BurgersGuidance(kw['shape'], kw['ori_shape'], resc, ut[b:b + 1], kw['wu'], kw['wf'])
        assert torch.equal(one(x_t[b:b + 1]), grad[b:b + 1]), b
        assert torch.equal(one.guide(mod, x_t[b:b + 1], eps[b:b + 1], t[b:b + 1], s_table, True), fused[b:b + 1]), b


# ----------------------------------------------------------------------------------------------------- chains
def _dif(trees, **over):
    with open(os.path.join(GOLDEN, 'ref_round2_manifest.json')) as f:
        m = json.load(f)['gb']
    u, d = m['unet'], dict(m['diffusion'])
    d['seq_length'] = tuple(d['seq_length'])
    d.update(over)
    net = trees['Unet2D'](dim=u['dim'], dim_mults=tuple(u['dim_mults']), channels=u['channels'], resnet_block_groups=u['resnet_block_groups'])
    dif = trees['GD1'](net, loss_layer_weight=torch.from_numpy(G2['gb::lw']), **d)
    sd = {k[len('gb::w::'):]: torch.from_numpy(G2[k]) for k in G2.files if k.startswith('gb::w::')}
    dif.load_state_dict({k: v for k, v in sd.items() if k.startswith('model.')}, strict=False)
    return dif.to(DEV)


def _chain_guidance(trees, u_target=None):
    c = GI.CHAIN
    ut, u_init, resc = GI.chain_input()
    g = trees['BG'].BurgersGuidance(c['shape'], c['ori'], resc, ut if u_target is None else u_target, c['wu'], c['wf'], condition_f=c['condition_f'])
    return g, u_init.to(DEV), ut.to(DEV), resc.to(DEV)


def _tape(tag):
    return iter([torch.from_numpy(G[f'chain::{tag}_noise_{i}']).to(DEV) for i in range(int(G[f'chain::{tag}_n_noise']))])


def _old_route(trees, ut, resc):
    c = GI.CHAIN
    return trees['MU'].get_nablaJ(lambda x: trees['BG'].guidance_value(x, ut, c['shape'], c['ori'], resc, c['wu'], c['wf'], c['condition_f']))


def test_guided_chains_vs_reference(trees):
    """DDIM-4 from t = 999 (cosine J schedule) and 6 ancestral steps (constant schedule) under the control objective, through
    sample(nablaJ=BurgersGuidance(...)), against the fp64 evaluation of the same chains. The DDIM chain amplifies last-bit differences by
    c2 = 1.8e3 at its first step (tests/test_gpu_round2.py:126-131), so it is gated by the arbiter like its smoke twin, not by a fixed bar."""
    g, u_init, _, _ = _chain_guidance(trees)
    dif = _dif(trees)
    seq = _tape('ddim')
    dif.sample_noise = lambda shape, device: next(seq)
    out = dif.sample(batch_size=2, u_init=u_init, nablaJ=g, J_scheduler=trees['MU'].get_scheduler('cosine'))
    h1, r1 = rel_l2(out, G['chain::ddim_out64']), rel_l2(G['chain::ddim_out'], G['chain::ddim_out64'])
    dif6 = _dif(trees, timesteps=6, sampling_timesteps=None)
    seq6 = _tape('ddpm6')
    dif6.sample_noise = lambda shape, device: next(seq6)
    out6 = dif6.sample(batch_size=2, u_init=u_init, nablaJ=g, J_scheduler=lambda t: GI.CHAIN['ddpm6_s'])
    h2, r2 = rel_l2(out6, G['chain::ddpm6_out64']), rel_l2(G['chain::ddpm6_out'], G['chain::ddpm6_out64'])
    print(f'guided chains vs fp64: ddim4 hip {h1:.3e} reference fp32 {r1:.3e} (hip vs reference {rel_l2(out, G["chain::ddim_out"]):.3e}) | '
          f'ddpm6 hip {h2:.3e} reference fp32 {r2:.3e} (hip vs reference {rel_l2(out6, G["chain::ddpm6_out"]):.3e})')
    assert A.gate(h1, r1), (h1, r1)
    assert A.gate(h2, r2), (h2, r2)


def _noises(n, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return [torch.randn(2, 9, 16, 16, device=DEV, generator=gen) for _ in range(n)]


def _run(dif, noises, **kw):
    seq = iter(noises)
    dif.sample_noise = lambda shape, device: next(seq)
    return dif.sample(batch_size=2, **kw)


@pytest.mark.parametrize('ddim', [False, True])
def test_graph_replay_equals_eager(trees, ddim):
    """12 noisy steps (past the capture threshold): the replayed loop and the eager launches return identical bits."""
    g, u_init, _, _ = _chain_guidance(trees)
    dif = _dif(trees, timesteps=1000 if ddim else 12, sampling_timesteps=13 if ddim else None)
    noises = _noises(13, 5)
    sched = trees['MU'].get_scheduler('cosine') if ddim else (lambda t: 0.1)
    dif.use_graph = True
    a = _run(dif, noises, u_init=u_init, nablaJ=g, J_scheduler=sched)
    assert len(trees['K']._graph_cache.get(dif, {})) == 1
    dif.use_graph = False
    b = _run(dif, noises, u_init=u_init, nablaJ=g, J_scheduler=sched)
    assert len(trees['K']._graph_cache.get(dif, {})) == 1 and torch.isfinite(a).all()
    assert torch.equal(a, b)
    # and the guidance is not a no-op on this chain
    c = _run(dif, noises, u_init=u_init)
    assert rel_l2(a, c) > 1e-3


def test_set_target_replays_the_captured_graph(trees):
    K = trees['K']
    g, u_init, ut, _ = _chain_guidance(trees)
    dif = _dif(trees, timesteps=12, sampling_timesteps=None)
    noises = _noises(12, 6)
    dif.use_graph = True
    a = _run(dif, noises, u_init=u_init, nablaJ=g, J_scheduler=lambda t: 0.1)
    graphs = dict(K._graph_cache[dif])
    assert len(graphs) == 1
    ut2 = ut.flip(0) * 0.5 + 0.25
    g.set_target(ut2)
    b = _run(dif, noises, u_init=u_init, nablaJ=g, J_scheduler=lambda t: 0.1)
    after = K._graph_cache[dif]
    assert len(after) == 1 and all(after[k] is v for k, v in graphs.items())        # one capture: the same _StepGraph served both calls
    g2, _, _, _ = _chain_guidance(trees, u_target=ut2)
    dif.use_graph = False
    c = _run(dif, noises, u_init=u_init, nablaJ=g2, J_scheduler=lambda t: 0.1)
    assert torch.equal(b, c) and not torch.equal(a, b)


def test_other_routes_are_unchanged(trees, monkeypatch):
    """Today's route -- nablaJ = get_nablaJ(guidance_value) through the eager loop -- still runs and lands where the new route does (both inside
    the arbiter gate of the 6-step chain); a custom proj_guidance keeps a BurgersGuidance on the eager loop."""
    K = trees['K']
    g, u_init, ut, resc = _chain_guidance(trees)
    dif6 = _dif(trees, timesteps=6, sampling_timesteps=None)
    sched = lambda t: GI.CHAIN['ddpm6_s']
    tape = [torch.from_numpy(G[f'chain::ddpm6_noise_{i}']).to(DEV) for i in range(6)]
    new = _run(dif6, tape, u_init=u_init, nablaJ=g, J_scheduler=sched)
    exact, r = G['chain::ddpm6_out64'], rel_l2(G['chain::ddpm6_out'], G['chain::ddpm6_out64'])
    monkeypatch.setattr(K, 'guided_sampling_loop_burgers', lambda *a, **k: (_ for _ in ()).throw(AssertionError('the fused loop was taken')))
    old = _run(dif6, tape, u_init=u_init, nablaJ=_old_route(trees, ut, resc), J_scheduler=sched)
    proj = _run(dif6, tape, u_init=u_init, nablaJ=g, J_scheduler=sched, proj_guidance=lambda ep, nj: ep + nj)
    hn, ho, hp = rel_l2(new, exact), rel_l2(old, exact), rel_l2(proj, exact)
    print(f'6-step guided chain vs fp64: new route {hn:.3e} autograd route {ho:.3e} BurgersGuidance on the eager loop {hp:.3e} reference fp32 {r:.3e}')
    assert A.gate(hn, r) and A.gate(ho, r) and A.gate(hp, r), (hn, ho, hp, r)
    # p_sample / model_predictions called directly take the object as the callable it is
    x = tape[0].clone()
    K.apply_cond(x, *dif6._sampling_setup(tuple(x.shape), dict(u_init=u_init)))
    a, _, _ = dif6.p_sample(x, 0, nablaJ=g, J_scheduler=sched)
    b, _, _ = dif6.p_sample(x, 0, nablaJ=_old_route(trees, ut, resc), J_scheduler=sched)
    assert rel_l2(a, b) < 1e-5
