"""The Burgers control-evaluation solver on the GPU (csrc/burgers.hip through wdno_amd.burgers_solver): reference fixtures under the arbiter
gate, bit-identity across configurations / batch positions / calls, a batch of 4 x CUs against an fp64 restatement, CPU and strided inputs."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.arbiter import gate
from tests.helpers import GOLDEN, rel_l2

pytestmark = pytest.mark.gpu

VISC = 0.01


def _manifest():
    with open(os.path.join(GOLDEN, 'ref_burgers_solver_manifest.json')) as f:
        return json.load(f)


M = _manifest()
_NPZ = {}


def _case(name):
    c = M['cases'][name]
    if c['file'] not in _NPZ:
        _NPZ[c['file']] = np.load(os.path.join(GOLDEN, c['file']))
    g = _NPZ[c['file']]
    return c, {k.split('/', 1)[1]: torch.from_numpy(g[k]) for k in g.files if k.startswith(name + '/')}


def _solve(*a, **k):
    from wdno_amd.burgers_solver import solve
    return solve(*a, **k)


def restated_fp64(u0, f, T, num_t, s=1920, dt=1 / 76800, visc=VISC):
    """generate_burgers.py:104-204 restated with slices in fp64 on u0's device (fp32 inputs and fp32-rounded constants): [N, num_t + 1, s]."""
    u = F.interpolate(u0.double()[:, None], size=s, mode='linear', align_corners=False)[:, 0]
    fi = F.interpolate(f.double(), size=s, mode='linear', align_corners=False)
    dx = 1.0 / (s + 1)
    c, d, dm = (float(np.float32(v)) for v in (1.0 / (2 * dx), visc * 1.0 / dx ** 2, visc * -2.0 / dx ** 2))
    dt32 = float(np.float32(dt))
    steps = math.ceil(T / dt)
    record_time, f_time = steps // num_t, steps // f.shape[1]
    out = torch.zeros(u.shape[0], num_t + 1, s, dtype=torch.float64, device=u.device)
    out[:, 0] = u
    up = torch.zeros(u.shape[0], s + 2, dtype=torch.float64, device=u.device)
    for j in range(steps):
        up[:, 1:-1] = u
        a, e = up[:, :-2], up[:, 2:]
        u = u + dt32 * (-0.5 * ((a * a) * (-c) + (e * e) * c) + (a * d + u * dm + e * d) + fi[:, j // f_time])
        if (j + 1) % record_time == 0:
            out[:, (j + 1) // record_time] = u
    return out


def _random_inputs(N, nx, Nt_f, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.linspace(0, 1, nx)
    loc, sig, amp = torch.rand(N, 1, generator=g), torch.rand(N, 1, generator=g) * 0.1 + 0.05, torch.rand(N, 1, generator=g) * 4 - 2
    u0 = amp * torch.exp(-0.5 * (x - loc) ** 2 / sig ** 2)
    f = torch.randn(N, Nt_f, 1, generator=g) * torch.exp(-0.5 * (x - torch.rand(N, 1, 1, generator=g)) ** 2 / 0.04)
    return u0.float().contiguous(), f.float().contiguous()


@pytest.mark.parametrize('name', ['A', 'B', 'C', 'D1', 'D2'])
def test_fixture_cases_arbiter_gate(name):
    """hip_vs_exact <= 1.5 ref_vs_exact + 1e-6 on the whole trajectory and on the final row alone (what J_actual reads); row 0 = torch's
    F.interpolate of u0 on the GPU."""
    c, g = _case(name)
    kw = dict(c['kwargs'])
    u0, f = g['u0'].cuda(), g['f'].cuda()
    out = _solve(u0, f, **kw)
    torch.cuda.synchronize()
    assert list(out.shape) == c['out_shape'] and out.dtype == torch.float32 and out.is_cuda
    sub = c['sub_s'] if kw.get('output_space_downsample', True) else 1
    row0 = F.interpolate(u0[:, None], size=kw.get('s', 1920), mode='linear', align_corners=False)[:, 0, ::sub]
    assert rel_l2(out[:, 0], row0) <= 1e-6
    if name == 'A':
        pairs = [(out[:, :, ::16], g['ref_cols16'], g['exact_d_cols16']), (out[:, -1], g['ref_last'], g['exact_d_last'])]
    else:
        pairs = [(out, g['ref'], g['exact_d']), (out[:, -1], g['ref'][:, -1], g['exact_d'][:, -1])]
    for hip, ref, d in pairs:
        exact = ref.double() + d.double()
        h, r = rel_l2(hip, exact), rel_l2(ref, exact)
        assert gate(h, r), (name, h, r)


def test_bit_identity_configs_positions_calls():
    """Every supported (W, P) gives the same bits; trajectory i alone equals trajectory i of the batch; two calls give the same bits."""
    from wdno_amd.burgers_solver import configs
    u0, f = _random_inputs(300, 120, 10, seed=5)
    u0, f = u0.cuda(), f.cuda()
    kw = dict(visc=VISC, T=0.05, num_t=10)
    base = _solve(u0, f, **kw)
    cfgs = configs(1920)
    assert len(cfgs) >= 10
    for cfg in cfgs:
        assert torch.equal(_solve(u0, f, config=cfg, **kw), base), cfg
    for i in (0, 137, 299):
        assert torch.equal(_solve(u0[i:i + 1], f[i:i + 1], **kw), base[i:i + 1]), i
    assert torch.equal(_solve(u0, f, **kw), base)
    assert torch.isfinite(base).all() and base[:, -1].abs().max() > 0


def test_restatement_matches_fixture_d():
    """The fp64 restatement used below reproduces the generator's independent fp64 evaluation (fixture cases D1, D2)."""
    for name in ('D1', 'D2'):
        c, g = _case(name)
        kw = c['kwargs']
        ex = restated_fp64(g['u0'].cuda(), g['f'].cuda(), kw['T'], kw['num_t'], s=kw.get('s', 1920))[:, :, ::c['sub_s']]
        assert rel_l2(ex, g['ref'].double() + g['exact_d'].double()) < 1e-9, name


def test_large_batch_one_wave_against_fp64():
    """N = 4 x CUs (more than one round of workgroups): the one-wave configuration, against the fp64 restatement."""
    from wdno_amd.burgers_solver import plan
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N = 4 * cus
    u0, f = _random_inputs(N, 120, 10, seed=11)
    u0, f = u0.cuda(), f.cuda()
    assert plan(tuple(u0.shape), tuple(f.shape), 0.05, num_t=10, cu_count=cus)['waves'] == 1
    out = _solve(u0, f, visc=VISC, T=0.05, num_t=10, output_space_downsample=False)
    ex = restated_fp64(u0, f, 0.05, 10)
    assert rel_l2(out, ex) < 1e-5                                      # fp32 rounding over 3 840 steps; a wrong stencil or halo is >= 1e-3
    assert rel_l2(out[:, -1], ex[:, -1]) < 1e-5


def test_cpu_and_strided_inputs():
    """CPU inputs come back on the CPU with the bits of the GPU-input result; u[:, 0] of a [N, T, nx] tensor (eval_ddpm_burgers.py:203)."""
    u, f = _random_inputs(6, 120, 10, seed=3)
    traj = torch.stack([u, u * 0.5], dim=1)                           # [N, 2, nx]: traj[:, 0] is not contiguous
    kw = dict(visc=VISC, T=0.05, num_t=10)
    gpu = _solve(u.cuda(), f.cuda(), **kw)
    cpu = _solve(traj[:, 0], f, **kw)
    assert cpu.device.type == 'cpu' and torch.equal(cpu, gpu.cpu())
    strided = _solve(traj.cuda()[:, 0], f.cuda().transpose(1, 2).contiguous().transpose(1, 2), **kw)
    assert torch.equal(strided, gpu)
    g = u.cuda().requires_grad_(True)
    assert not _solve(g, f.cuda(), **kw).requires_grad


def test_dropin_is_the_hip_solver():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('_dropin_generate_burgers_gpu',
                                                  os.path.join(root, 'wdno_amd', 'burgers', 'ddpm_burgers', 'generate_burgers.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    u, f = _random_inputs(3, 120, 10, seed=9)
    a = mod.burgers_numeric_solve_free(u.cuda(), f.cuda(), visc=VISC, T=0.05, num_t=10)
    assert torch.equal(a, _solve(u.cuda(), f.cuda(), visc=VISC, T=0.05, num_t=10))
    assert a.shape == (3, 11, 120)
