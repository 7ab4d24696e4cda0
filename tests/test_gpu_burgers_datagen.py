"""The Burgers data-set generator on the GPU (csrc/burgers_datagen.hip through wdno_amd.burgers_datagen): the same bits as the solver kernel
on the dense forcing for every configuration, the tables against the reference's expressions, batch independence, the data-set shape, no
dense forcing in memory, an fp64 restatement that does not involve the solver kernel, and the files end to end."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests.arbiter import gate
from tests.helpers import GOLDEN, rel_l2

pytestmark = pytest.mark.gpu

VISC = 0.01
T_SHORT = 0.01          # 768 steps
with open(os.path.join(GOLDEN, 'ref_burgers_datagen_manifest.json')) as _f:
    ALPHA = json.load(_f)['alpha']          # the fixture's alpha, at which the clamp at +-10 is active
_DRAWS = {}


def _draw(N, s, t, seed=0):
    """A seeded draw on the GPU, made once per (N, s, t, seed) and shared (never written to)."""
    from wdno_amd.burgers_datagen import draw
    key = (N, s, t, seed)
    if key not in _DRAWS:
        torch.manual_seed(1234 + seed)
        _DRAWS[key] = draw(N, s, t, 'cuda')
    return _DRAWS[key]


def _check_against_solver(N, s, t, nx, nt, num_t, T, alpha=1., cfgs=None):
    """generate() for every configuration (or those of `cfgs`) and for the one plan() chooses, against solve() on the dense forcing and
    the dense forcing's own slice, with torch.equal."""
    from wdno_amd import burgers_datagen as D, burgers_solver as B
    u0, AX, TT = _draw(N, s, t)
    f = D.dense_forcing(AX, TT, alpha)
    sx, st = int(s / nx), int(t / nt)
    want_u = B.solve(u0, f, VISC, T, num_t=num_t, s=s, output_space_downsample=False)[:, :, ::sx]
    want_f = f[:, ::st, ::sx]
    assert torch.equal(want_u[:, 0], u0[:, ::sx])
    cfgs = B.configs(s) if cfgs is None else cfgs
    for cfg in cfgs:
        u_rec, f_rec = D.generate(u0, AX, TT, T, num_t, nx, nt, alpha=alpha, config=cfg)
        assert u_rec.shape == want_u.shape and f_rec.shape == want_f.shape and u_rec.dtype == f_rec.dtype == torch.float32
        assert torch.equal(u_rec, want_u), cfg
        assert torch.equal(f_rec, want_f), cfg
        assert torch.equal(u_rec[:, 0], u0[:, ::sx]), cfg
    u_rec, f_rec = D.generate(u0, AX, TT, T, num_t, nx, nt, alpha=alpha)          # the configuration plan() chooses
    assert torch.equal(u_rec, want_u) and torch.equal(f_rec, want_f)
    assert torch.isfinite(u_rec).all() and u_rec[:, -1].abs().max() > 0
    return u_rec, f_rec


@pytest.mark.parametrize('s, t, nx, nt, num_t', [
    (200, 24, 50, 4, 4),
    (333, 6, 100, 3, 3),            # a partial last wave, strides that do not divide
    (1920, 768, 120, 48, 8),        # f_time = 1: a new interval every step
])
def test_same_bits_as_solver_on_dense_forcing(s, t, nx, nt, num_t):
    _check_against_solver(5, s, t, nx, nt, num_t, T_SHORT)


def test_same_bits_as_solver_with_clamp():
    _, f_rec = _check_against_solver(5, 200, 24, 50, 4, 4, T_SHORT, alpha=ALPHA)
    assert (f_rec.abs() == 10.).any() and (f_rec.abs() < 10.).any()


def test_tables_match_reference_form_on_gpu():
    """dense_forcing of a GPU draw against make_data_varying_f's expressions (generate_burgers.py:223-270) restated with their `.repeat`s on
    the same seeded draws."""
    from wdno_amd.burgers_datagen import dense_forcing, draw
    Nf, s, t, device, amp_compensate = 3, 120, 80, 'cuda', 2
    torch.manual_seed(77)
    u0, AX, TT = draw(Nf, s, t, device)
    torch.manual_seed(77)
    x = torch.linspace(1.0 / (s + 1), 1.0 - 1.0 / (s + 1), s).to(device)
    ts = torch.linspace(1.0 / (t + 1), 1.0 - 1.0 / (t + 1), t).to(device)
    loc1 = torch.rand(Nf, 1, device=device) * 0.2 + 0.2
    amp1 = torch.rand(Nf, 1, device=device) * 2
    sig1 = torch.rand(Nf, 1, device=device) * 0.1 + 0.05
    gauss1 = amp1 * torch.exp(-0.5 * (x.view(1, -1) - loc1) ** 2 / sig1 ** 2)
    loc2 = torch.rand(Nf, 1, device=device) * 0.2 + 0.6
    amp2 = torch.rand(Nf, 1, device=device) * 2 - 2
    sig2 = torch.rand(Nf, 1, device=device) * 0.1 + 0.05
    gauss2 = amp2 * torch.exp(-0.5 * (x.view(1, -1) - loc2) ** 2 / sig2 ** 2)

    def rand_f(is_rand_amp):
        if is_rand_amp:
            amp = torch.randint(2, (Nf, 1, 1), device=device).float() * (torch.rand(Nf, 1, 1, device=device) * 3 - 1.5)
        else:
            amp = (torch.rand(Nf, 1, 1, device=device) * 3 - 1.5)
        amp = amp.repeat(1, t, s)
        loc = torch.rand(Nf, 1, 1, device=device)
        sig = torch.rand(Nf, 1, 1, device=device) * 0.3 + 0.1
        exp_space = torch.exp(-0.5 * (x.view(1, 1, -1).repeat(Nf, t, 1) - loc) ** 2 / sig ** 2)
        loc = torch.rand(Nf, 1, 1, device=device)
        sig = torch.rand(Nf, 1, 1, device=device) * 0.3 + 0.1
        exp_time = amp_compensate * torch.exp(-0.5 * (ts.view(1, -1, 1).repeat(Nf, 1, s) - loc) ** 2 / sig ** 2)
        return amp * exp_space * exp_time
    f = rand_f(False)
    for _ in range(7):
        f += rand_f(True)
    assert torch.equal(u0, gauss1 + gauss2)
    assert torch.equal(dense_forcing(AX, TT), f.to(torch.float32))
    assert torch.equal(dense_forcing(AX, TT, ALPHA), (f * ALPHA).clamp(-10., 10.))


def test_batch_independence_and_repeatability():
    from wdno_amd.burgers_datagen import generate
    u0, AX, TT = _draw(300, 200, 24, seed=1)
    kw = dict(T=T_SHORT, num_t=4, nx=50, nt=4)
    u_rec, f_rec = generate(u0, AX, TT, **kw)
    for i in (0, 137, 299):
        u1, f1 = generate(u0[i:i + 1], AX[i:i + 1], TT[i:i + 1], **kw)
        assert torch.equal(u1, u_rec[i:i + 1]) and torch.equal(f1, f_rec[i:i + 1]), i
    u2, f2 = generate(u0, AX, TT, **kw)
    assert torch.equal(u2, u_rec) and torch.equal(f2, f_rec)
    assert torch.isfinite(u_rec).all() and torch.isfinite(f_rec).all()
    assert (u_rec[:, -1].abs().amax(dim=1) > 0).all()


def test_data_set_shape():
    """The reference's data-set call itself (s = 1920, t = 1280, T = 8, nt = 80, nx = 120: 614 400 steps, 480 per interval) on two trajectories:
    the configuration of a batch of 800, the one plan() takes for two trajectories, and one wave per trajectory (0.2 - 0.4 s each; the
    other configurations run the same code at 768 steps above)."""
    from wdno_amd.burgers_datagen import choose_config
    cfgs = sorted({choose_config(800, 1920), (1, 32)})
    assert (2, 16) in cfgs
    u_rec, f_rec = _check_against_solver(2, 1920, 1280, 120, 80, 80, 8, cfgs=cfgs)
    assert u_rec.shape == (2, 81, 120) and f_rec.shape == (2, 80, 120)


def test_no_dense_forcing_in_memory():
    """generate() allocates its outputs and nothing of the size of f: the peak rises by at most twice the outputs' bytes (a dense f of this
    call is 79 MB, the outputs are 0.6 MB)."""
    from wdno_amd.burgers_datagen import generate
    u0, AX, TT = _draw(8, 1920, 1280)
    kw = dict(T=0.05, num_t=80, nx=120, nt=80)          # 3 840 steps, 3 per interval
    generate(u0, AX, TT, **kw)                             # the library is loaded, the inputs exist
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    u_rec, f_rec = generate(u0, AX, TT, **kw)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    out_bytes = u_rec.numel() * 4 + f_rec.numel() * 4
    assert u_rec.shape == (8, 81, 120) and f_rec.shape == (8, 80, 120)
    assert rise <= 2 * out_bytes, (rise, out_bytes)


# ------------------------------------------------------------------------------------------ independent of the solver kernel
def _parameters(N, seed):
    """The fp32 draws of make_data_varying_f in its call order, from a CPU generator: what the tables are functions of."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.rand(*shape, generator=g)
    p = dict(loc1=r(N, 1) * 0.2 + 0.2, amp1=r(N, 1) * 2, sig1=r(N, 1) * 0.1 + 0.05,
             loc2=r(N, 1) * 0.2 + 0.6, amp2=r(N, 1) * 2 - 2, sig2=r(N, 1) * 0.1 + 0.05, terms=[])
    for k in range(8):
        if k:
            amp = torch.randint(2, (N, 1, 1), generator=g).float() * (r(N, 1, 1) * 3 - 1.5)
        else:
            amp = r(N, 1, 1) * 3 - 1.5
        p['terms'].append(dict(amp=amp, loc_x=r(N, 1, 1), sig_x=r(N, 1, 1) * 0.3 + 0.1, loc_t=r(N, 1, 1), sig_t=r(N, 1, 1) * 0.3 + 0.1))
    return p


def _tables(p, s, t, dtype):
    """u0 [N, s], AX [N, 8, s], TT [N, t, 8] of the fp32 parameters p, every operation in `dtype` on the GPU (the fp32 grid points widened)."""
    c = lambda v: v.to('cuda', dtype)
    x = c(torch.linspace(1.0 / (s + 1), 1.0 - 1.0 / (s + 1), s))
    ts = c(torch.linspace(1.0 / (t + 1), 1.0 - 1.0 / (t + 1), t))
    u0 = c(p['amp1']) * torch.exp(-0.5 * (x.view(1, -1) - c(p['loc1'])) ** 2 / c(p['sig1']) ** 2) + \
        c(p['amp2']) * torch.exp(-0.5 * (x.view(1, -1) - c(p['loc2'])) ** 2 / c(p['sig2']) ** 2)
    ax = [c(q['amp']) * torch.exp(-0.5 * (x.view(1, 1, -1) - c(q['loc_x'])) ** 2 / c(q['sig_x']) ** 2) for q in p['terms']]
    tt = [2 * torch.exp(-0.5 * (ts.view(1, -1, 1) - c(q['loc_t'])) ** 2 / c(q['sig_t']) ** 2) for q in p['terms']]
    return u0, torch.cat(ax, dim=1), torch.cat(tt, dim=2)


def _chain(u0, AX, TT, T, num_t, dtype, dt=1 / 76800, visc=VISC):
    """The whole chain in `dtype` with slices: the forcing summed from the tables, generate_burgers.py:176-195 with fp32-rounded constants
    (l.163-165). [N, num_t + 1, s]."""
    s, t = u0.shape[1], TT.shape[1]
    f = sum(AX[:, k, None, :] * TT[:, :, k, None] for k in range(8)).to(dtype)
    dx = 1.0 / (s + 1)
    c, d, dm = (float(np.float32(v)) for v in (1.0 / (2 * dx), visc * 1.0 / dx ** 2, visc * -2.0 / dx ** 2))
    dt32 = float(np.float32(dt))
    steps = math.ceil(T / dt)
    record_time, f_time = steps // num_t, steps // t
    u = u0.to(dtype)
    out = torch.zeros(u.shape[0], num_t + 1, s, dtype=dtype, device=u.device)
    out[:, 0] = u
    up = torch.zeros(u.shape[0], s + 2, dtype=dtype, device=u.device)
    for j in range(steps):
        up[:, 1:-1] = u
        a, e = up[:, :-2], up[:, 2:]
        u = u + dt32 * (-0.5 * ((a * a) * (-c) + (e * e) * c) + (a * d + u * dm + e * d) + f[:, j // f_time])
        if (j + 1) % record_time == 0:
            out[:, (j + 1) // record_time] = u
    return out


def test_against_fp64_restatement_arbiter_gate():
    """hip_vs_exact <= 1.5 ref_vs_exact + 1e-6 on u_rec and on its last row. Exact: the chain in fp64, tables included, from the fp32
    parameters. Reference: the same restatement in fp32. The kernel is fed the fp32 tables."""
    from wdno_amd.burgers_datagen import generate
    N, s, t, nx, nt, num_t = 16, 200, 24, 50, 4, 4
    p = _parameters(N, seed=5)
    u0, AX, TT = _tables(p, s, t, torch.float32)
    hip, _ = generate(u0, AX, TT, T_SHORT, num_t, nx, nt)
    sx = int(s / nx)
    ref = _chain(u0, AX, TT, T_SHORT, num_t, torch.float32)[:, :, ::sx]
    exact = _chain(*_tables(p, s, t, torch.float64), T_SHORT, num_t, torch.float64)[:, :, ::sx]
    assert exact[:, -1].abs().max() > 0
    for a, b, e in ((hip, ref, exact), (hip[:, -1], ref[:, -1], exact[:, -1])):
        h, r = rel_l2(a, e), rel_l2(b, e)
        print(f'hip_vs_exact {h:.3e} ref_vs_exact {r:.3e}')
        assert gate(h, r), (h, r)


def test_write_dataset_end_to_end(tmp_path):
    from wdno_amd.burgers_datagen import write_dataset
    save = str(tmp_path) + os.sep
    n = write_dataset(save, 12, 4, batch_size=8, end_time=T_SHORT, nt=4, nx=50, alpha=1., seed=3, s=200, t=24)
    assert n == (12, 4)
    for name, cnt in (('train', 12), ('test', 4)):
        d = torch.load(save + name)
        assert d['u'].shape == (cnt, 5, 50) and d['f'].shape == (cnt, 4, 50)
        assert d['u'].dtype == d['f'].dtype == torch.float32 and d['u'].device.type == 'cpu'
        assert torch.isfinite(d['u']).all() and torch.isfinite(d['f']).all()
        assert (d['u'][:, 0].abs().amax(dim=1) > 0).all() and (d['u'][:, -1].abs().amax(dim=1) > 0).all()
    with pytest.raises(FileExistsError):
        write_dataset(save, 12, 4, batch_size=8, end_time=T_SHORT, nt=4, nx=50, seed=3, s=200, t=24)
