"""GroupNorm(+scale/shift)(+SiLU)(+residual) and its backward in plain torch on the CPU, fp64, with an ERROR SCALE for every output.
Test infrastructure only: the operation wdno_amd/csrc/norm.hip implements (its header comment, gn_finalize_kernel and
gn_bwd_finalize_kernel define the fold), checked against F.group_norm and autograd by tests/test_host_groupnorm_ref.py.

Layout: channels-last x [N, S, C], gamma / beta [C], scale_shift [N, 2C] (scale in [:, :C], shift in [:, C:]), G groups of cg = C / G
channels. All inputs are fp32 values, upcast exactly. With mu, rstd the statistics of a (sample, group), s the scale, sh the shift:

    k1 = rstd gamma        a = k1 (s + 1)        b = (beta - mu k1)(s + 1) + sh        z = a x + b        y = act(z)
    dz = dy act'(z)        A = sum_s dz          B = sum_s dz xhat                      xhat = (x - mu) rstd
    dgamma = sum_n (s + 1) B    dbeta = sum_n (s + 1) A    dscale = gamma B + beta A    dshift = A
    g.z = rstd mean_group(gamma (s + 1) A)      g.w = rstd mean_group(gamma (s + 1) B)
    dx = a dz - g.z - xhat g.w                   colsum = sum_(n, s) dx

THE GATE is element-wise:  |got - ref| <= K * 2^-24 * scale.  `scale` is the sum of the absolute values of the terms the kernel's own
formula adds, in fp64, so a result that cancels (y = a x + b on an input with mean 20 and std 0.5) is held to the rounding of its terms
and not to its own size:

    zs  (pre-activation) = |a x| + |beta (s + 1)| + |mu k1 (s + 1)| + |sh|
    y                    = zs + |y|                       (y + residual: + |y + residual|)
    xs  (xhat)           = (|x| + |mu|) rstd
    es  (dz)             = |dz| + |dy| zs                 (second term with SiLU only: act'(z) = sg (1 + z (1 - sg)) is evaluated at a z that
                                                           carries zs 2^-24 of rounding, and its 1 - sg cancels; this is the |dy| |z|-sized
                                                           term, with |z| taken as the sum of |terms| of z so that it also holds where z cancels)
    eb  (dz xhat)        = es |xhat| + |dz| xs            (first order: the rounding of each factor times the size of the other)
    gzs, gws             = rstd mean_group(|gamma (s + 1)| sum_s es), rstd mean_group(|gamma (s + 1)| sum_s eb)
                           (g.z and g.w are means of signed terms: over a small group -- cg S = 72 in the matrix -- they cancel to
                           far below the rounding of their terms, so their own size says nothing about their error. Measured: with |g.z|, |g.w|
                           and |dy| |z| in their place the transcription itself is at ratio 58.8 on (256, 9, 64, 8) and 52.2 on
                           (2, 70, 512, 128), which would put K near 240; with the sums of |terms| it is at 3.43)
    dx                   = |a| es + gzs + |xhat| gws + xs |g.w|
    dbeta  = sum |s + 1| es                dgamma = sum |s + 1| eb
    dshift = sum es                        dscale = sum (|gamma| eb + |beta| es)
    colsum = sum (scale of dx)

K, one per output kind, is NOT taken from the kernels: transcription() below is the kernels' formulas in fp32 torch (fp64 statistics and
sums as the kernels keep them, fp32 a, b and apply). Its worst ratio |got - ref| / (2^-24 scale) over the whole case matrix (CASES x
variants x act on / off x scale-shift on / off, tests/test_host_groupnorm_ref.py re-measures it and holds it to K / 2) is

    MEASURED = {y: 2.39, y_add: 2.15, dx: 3.43, param: 1.51, dss: 1.74, colsum: 0.78}

and K = ceil(4 x that): the device's expf and division are a few ulp where the host's are at most 1, and a compiler that contracts
a x + b (and the three terms of dx) into FMAs moves single roundings (wdno_amd/build.py pins -ffp-contract=off today; the gate does
not depend on it).

    K = {y: 10, y_add: 9, dx: 14, param: 7, dss: 7, colsum: 4}

Planes. plane_pack (csrc/common.h) stores t = v * scale (exact: scale is a power of two) as hi = fp16(t), lo = fp16(t - hi). |t| < 2^15,
so |t - hi| <= 2^-11 |t| and t - hi is exact in fp32; lo then rounds it with relative error 2^-11 while it is a normal fp16 (|lo| >= 2^-14)
and with absolute error <= 2^-25 below. So |(hi + lo) / scale - v| <= 2^-22 |v| + 2^-25 / scale; the tests allow twice that,
2^-21 |v| + 2^-24 / scale (REP), on top of the gate of the fp32 value v.
"""
import functools
import math

import torch

EPS = float(torch.tensor(1e-5, dtype=torch.float32))        # the eps the library receives (a C float), upcast exactly
U = 2.0 ** -24

# measured by tests/test_host_groupnorm_ref.py::test_transcription_stays_within_half_the_gate (see the module docstring)
K = {'y': 10, 'y_add': 9, 'dx': 14, 'param': 7, 'dss': 7, 'colsum': 4}
KIND = {'y': 'y', 'y_add': 'y_add', 'dx': 'dx', 'dgamma': 'param', 'dbeta': 'param', 'dss': 'dss', 'colsum': 'colsum'}

# (N, S, C, G): nchunk the library must choose, rows of column-sum partials of the planes backward (None: C / 8 is no power of two, no
# planes forms), and whether only a reduced set of (act, scale_shift) combinations runs (the two large cases)
CASES = [
    ((2, 300, 64, 8), 5, 2 * 10, False),          # anchor. 8 slices of one group
    ((3, 130, 24, 4), 3, None, False),            # 6 lanes of txp 8; nsub = 42; odd nchunk
    ((2, 177, 8, 8), 3, 2 * 1, False),            # cg = 1: a slice is one channel, nsub = 256; C8 = 1
    ((2, 177, 8, 1), 3, 2 * 1, False),
    ((5, 37, 4, 1), 1, None, False),              # txp = 1, nty = 256, fewer rows than row groups
    ((5, 37, 4, 4), 1, None, False),
    ((1, 1, 8, 1), 1, 1, False),                  # S = 1
    ((2, 3, 1024, 32), 1, 2 * 2, False),          # 32 slices; cg = 32; three rows; txp 256
    ((3, 161, 128, 2), 3, 3 * 11, False),         # cg = 64, the last serial-sum width; nsub = 4 with nchunk 3
    ((2, 97, 136, 2), 4, None, False),            # cg = 68, the first block-reduced width, two groups
    ((3, 161, 256, 2), 6, 3 * 21, False),         # cg = 128, two wide groups
    ((2, 97, 1020, 1), 16, None, False),          # 255 of 256 lanes; cg no multiple of 256
    ((2, 70, 264, 33), 8, None, False),           # G >= 32: gps = 2, 17 live slices, last slice one group
    ((2, 70, 512, 128), 8, 2 * 18, False),        # gps = 4; cg = 4: a planes thread spans two groups
    ((2, 70, 256, 64), 4, 2 * 9, False),          # gps = 2; cg = 4
    ((2, 515, 256, 1), 18, 2 * 65, False),        # unrolled-8 twice, then a pair; planes grid 65
    ((1, 1200, 256, 8), 38, 128, False),          # 38 chunks over nsub = 8: pieces of 4 and 5
    ((1, 4100, 32, 8), 64, 65, False),            # rows per chunk 65, last chunk 5 rows
    ((1, 16384, 64, 8), 256, 128, True),          # N = 1: nchunk 256; unrolled-8 inside sliced totals; planes grid at its cap
    ((1, 2048, 1024, 1), 256, 128, True),         # nchunk 256 at nsub = 1
    ((256, 9, 64, 8), 1, 256 * 1, False),         # N > 64: bound-record slot wrap; sample sum over 256 rows
]
ANCHOR = (2, 300, 64, 8)
# (case, variant): 'std' = mean 0.7, std 2; 'mean20' = mean 20, std 0.5 (the fold cancels); 'const' = one group of one sample constant
MATRIX = [(c[0], 'std') for c in CASES] + [(ANCHOR, 'mean20'), ((3, 161, 256, 2), 'mean20'), (ANCHOR, 'const')]
CASE_INFO = {c[0]: c for c in CASES}


def case_id(cv):
    (n, s, c, g), v = cv
    return f'{n}x{s}x{c}g{g}' + ('' if v == 'std' else '-' + v)


def configs(case):
    """(act, use_ss) combinations a case runs."""
    return [(True, True), (False, False)] if CASE_INFO[case][3] else [(True, True), (True, False), (False, True), (False, False)]


def planes_ok(c):
    return c % 8 == 0 and c // 8 <= 256 and (c // 8) & (c // 8 - 1) == 0


@functools.lru_cache(maxsize=4)
def inputs(case, variant='std'):
    """fp32 CPU tensors of a case: x, gamma, beta, ss, res, dy (treat them as read-only: they are shared)."""
    n, s, c, g = case
    gen = torch.Generator().manual_seed(1000 * n + 7 * s + 3 * c + g)
    r = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)
    x = r(n, s, c) * 2 + 0.7
    if variant == 'mean20':
        x = (x - 0.7) * 0.25 + 20
    elif variant == 'const':
        x[0, :, :c // g] = 0.7
    out = dict(x=x, gamma=1 + 0.3 * r(c), beta=0.3 * r(c), ss=0.5 * r(n, 2 * c), res=r(n, s, c), dy=r(n, s, c))
    return {k: v.float() for k, v in out.items()}


def _per_channel(t, cg):
    return t.repeat_interleave(cg, dim=1)


def reference(x, gamma, beta, groups, ss=None, act=True, residual=None, dy=None, eps=EPS):
    """fp64 outputs and their error scales: ({name: tensor}, {name: scale}, info). y (+ y_add with a residual); with dy also dx, dgamma,
    dbeta, dss (None without ss) and colsum. info: the analytic bounds the planes kernels may use, and max|.| of y and dx."""
    n, s, c = x.shape
    cg = c // groups
    xd, gam, bet = x.double(), gamma.double(), beta.double()
    xg = xd.reshape(n, s, groups, cg)
    mean = xg.mean(dim=(1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean(dim=(1, 3))
    rstd = 1.0 / torch.sqrt(var + eps)
    mu, rs = _per_channel(mean, cg), _per_channel(rstd, cg)                       # [N, C]
    sc1 = ss.double()[:, :c] + 1 if ss is not None else torch.ones(n, c, dtype=torch.float64)
    sh = ss.double()[:, c:] if ss is not None else torch.zeros(n, c, dtype=torch.float64)
    k1 = rs * gam
    a = k1 * sc1
    b = (bet - mu * k1) * sc1 + sh
    xhat = (xd - mu[:, None]) * rs[:, None]
    z = (xhat * gam + bet) * sc1[:, None] + sh[:, None]
    sg = torch.sigmoid(z)
    y = z * sg if act else z
    zs = (a[:, None] * xd).abs() + ((bet * sc1).abs() + (mu * k1 * sc1).abs() + sh.abs())[:, None]
    out, scale = {'y': y}, {'y': zs + y.abs()}
    info = {'bound_y': float(a.abs().max() * xd.abs().max() + b.abs().max()), 'amax_y': float(y.abs().max())}
    if residual is not None:
        out['y_add'] = y + residual.double()
        scale['y_add'] = zs + y.abs() + out['y_add'].abs()
    if dy is None:
        return out, scale, info
    dyd = dy.double()
    dz = dyd * (sg * (1 + z * (1 - sg))) if act else dyd
    es = dz.abs() + dyd.abs() * zs if act else dz.abs()
    xs = (xd.abs() + mu.abs()[:, None]) * rs[:, None]
    A, B = dz.sum(1), (dz * xhat).sum(1)                                          # [N, C]
    eA, eB = es.sum(1), (es * xhat.abs() + dz.abs() * xs).sum(1)             # first order: d(dz xhat) = d(dz) xhat + dz d(xhat)
    out['dgamma'], scale['dgamma'] = (sc1 * B).sum(0), (sc1.abs() * eB).sum(0)
    out['dbeta'], scale['dbeta'] = (sc1 * A).sum(0), (sc1.abs() * eA).sum(0)
    if ss is not None:
        out['dss'] = torch.cat([gam * B + bet * A, A], dim=1)
        scale['dss'] = torch.cat([gam.abs() * eB + bet.abs() * eA, eA], dim=1)
    w = gam * sc1
    m = float(cg * s)
    gz = (w * A).reshape(n, groups, cg).sum(2) / m * rstd
    gw = (w * B).reshape(n, groups, cg).sum(2) / m * rstd
    gzc, gwc = _per_channel(gz, cg)[:, None], _per_channel(gw, cg)[:, None]
    dx = a[:, None] * dz - gzc - xhat * gwc
    out['dx'] = dx
    sgz = (w.abs() * eA).reshape(n, groups, cg).sum(2) / m * rstd                # g.z, g.w as sums of |terms|: means over a group cancel
    sgw = (w.abs() * eB).reshape(n, groups, cg).sum(2) / m * rstd
    sgzc, sgwc = _per_channel(sgz, cg)[:, None], _per_channel(sgw, cg)[:, None]
    scale['dx'] = a.abs()[:, None] * es + sgzc + xhat.abs() * sgwc + xs * gwc.abs()
    out['colsum'], scale['colsum'] = dx.sum((0, 1)), scale['dx'].sum((0, 1))
    info['bound_dx'] = float(a.abs().max() * dz.abs().max() + gz.abs().max() + xhat.abs().max() * gw.abs().max())
    info['amax_dx'] = float(dx.abs().max())
    return out, scale, info


@functools.lru_cache(maxsize=8)
def reference_of(case, variant, act, use_ss):
    """reference() of a case of the matrix with residual and dy, computed once and shared (read-only)."""
    t = inputs(case, variant)
    return reference(t['x'], t['gamma'], t['beta'], case[3], t['ss'] if use_ss else None, act, t['res'], t['dy'])


def transcription(x, gamma, beta, groups, ss=None, act=True, residual=None, dy=None, eps=EPS, rstd_error=None, drop_row=None):
    """The kernels' formulas in fp32 torch: statistics and sums over rows / samples in fp64 (as the kernels accumulate them), the tables
    a, b, k1 and every per-element step in fp32, one rounding per operation. Returns {name: fp32 tensor} like reference().
    rstd_error = (n, g, rel): that group's rstd is wrong by the relative amount rel. drop_row = (n, r): row r of sample n is left out of
    every sum over rows. Both exist to show that the gate sees such faults (tests/test_host_groupnorm_ref.py)."""
    n, s, c = x.shape
    cg = c // groups
    f32 = torch.float32
    x, gamma, beta = x.to(f32), gamma.to(f32), beta.to(f32)
    keep = torch.ones(n, s, 1, dtype=torch.float64)
    if drop_row is not None:
        keep[drop_row[0], drop_row[1]] = 0
    xd = x.double()
    m = float(cg * s)
    s0 = (xd * keep).sum(1).reshape(n, groups, cg).sum(2)
    s1 = (xd * xd * keep).sum(1).reshape(n, groups, cg).sum(2)
    mean = s0 / m
    var = (s1 / m - mean * mean).clamp_min(0)
    rstd = (1.0 / torch.sqrt(var + eps)).to(f32)
    mean = mean.to(f32)
    if rstd_error is not None:
        rstd[rstd_error[0], rstd_error[1]] *= torch.tensor(1.0 + rstd_error[2], dtype=f32)
    mu, rs = _per_channel(mean, cg), _per_channel(rstd, cg)
    sc1 = ss.to(f32)[:, :c] + 1.0 if ss is not None else torch.ones(n, c, dtype=f32)
    sh = ss.to(f32)[:, c:] if ss is not None else torch.zeros(n, c, dtype=f32)
    k1 = rs * gamma
    a = k1 * sc1
    b = (beta - mu * k1) * sc1 + sh
    z = a[:, None] * x + b[:, None]
    y = z / (1.0 + torch.exp(-z)) if act else z
    out = {'y': y}
    if residual is not None:
        out['y_add'] = y + residual.to(f32)
    if dy is None:
        return out
    dz = dy.to(f32)
    if act:
        sg = 1.0 / (1.0 + torch.exp(-z))
        dz = dz * (sg * (1.0 + z * (1.0 - sg)))
    xh = (x - mu[:, None]) * rs[:, None]
    A = (dz.double() * keep).sum(1)
    B = (dz.double() * xh.double() * keep).sum(1)
    gd, bd, sd = gamma.double(), beta.double(), sc1.double()
    out['dgamma'] = (sd * B).to(f32).double().sum(0).to(f32)          # per-sample pieces are stored as fp32, then summed in fp64
    out['dbeta'] = (sd * A).to(f32).double().sum(0).to(f32)
    if ss is not None:
        out['dss'] = torch.cat([(gd * B + bd * A).to(f32), A.to(f32)], dim=1)
    w = gd * sd
    gz = ((w * A).reshape(n, groups, cg).sum(2) / m).to(f32) * rstd
    gw = ((w * B).reshape(n, groups, cg).sum(2) / m).to(f32) * rstd
    dx = a[:, None] * dz - _per_channel(gz, cg)[:, None] - xh * _per_channel(gw, cg)[:, None]
    out['dx'] = dx
    out['colsum'] = dx.double().sum((0, 1)).to(f32)
    return out


def ratio(got, ref, scale, extra=None):
    """max of |got - ref| / (2^-24 scale); `extra` is an absolute allowance taken off the error first (REP of a planes pair)."""
    err = (got.detach().double().cpu().reshape(ref.shape) - ref).abs()
    if extra is not None:
        err = (err - extra).clamp_min(0)
    r = err / (U * scale).clamp_min(1e-300)
    return float(r.max()) if torch.isfinite(r).all() else math.inf


def ratios(got, ref):
    """{name: ratio} for every output of `got` (a dict like reference()'s first) against ref = (out, scale, info)."""
    return {k: ratio(v, ref[0][k], ref[1][k]) for k, v in got.items() if v is not None}


def rep_allowance(v, plane_scale):
    """REP of the module docstring for fp64 values v stored as an fp16 plane pair of the given scale."""
    return 2.0 ** -21 * v.abs() + 2.0 ** -24 / plane_scale
