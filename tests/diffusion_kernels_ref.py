"""fp64 reference, error scale, gate and case matrix for the kernels of csrc/diffusion.hip: q_sample with the conditioning masks and apply_cond,
the weighted MSE with its fused and its separate gradient, and the DDPM / DDIM / DDIM-dev sampler updates.

REFERENCE. numpy, written from the formulas and from no kernel; one statement of each formula runs in three arithmetics (`Arith`): float64 (the
reference), float32 with every product and every add rounded, and float32 with each product-then-add fused (a contracting compiler) -- the two
TRANSCRIPTIONS that show, on the host, that K holds for a correct fp32 implementation (tests/test_host_diffusion_kernels_ref.py).
    q_sample : x = sa[t_b] x0 + sb[t_b] noise; masks from oracle/diffusion_ref.py (smoke_apply_conditions, burgers_apply_conditions: the
               reference's statement order, later statements win), applied to marker tensors -> code 0 free, 1 zero, 2 clean. `cond_table` is an
               independent per-element statement of the same rules (priority selection), checked against the oracle's functions on the host.
    loss     : sum_e (out - tgt)^2 wc[c(e)] wb[b(e)] inv_count, c(e) = (e / inner) % C over [B][F][C][inner]; inv_count = fp32(1 / numel), the
               value the library receives. grad = 2 (out - tgt) wc wb inv_count gscale.
    DDPM     : st = clamp(c1[t] x - c2[t] eps); x_next = m1[t] st + m2[t] x + exp(lv[t] / 2) noise     (oracle: posterior_step)
    DDIM     : a = c1[t] x; st = clamp(a - c2[t] eps); eps' = (a - st) / c2[t]; x_next = st sqrt_an + c eps' + sigma noise (oracle: ddim_update)
Tables, t, weights and the three DDIM scalars enter as the fp32 values the library receives.

GATE. |got - ref| <= K 2^-24 S_e. S_e is the same formula on absolute values with every subtraction turned into an addition; K is the number of
roundings on the path to that output plus one for second-order terms:
    q_sample x        2 products + 1 add                                                   3 + 1 = K_Q        4
    x_start           2 products + 1 subtraction (both samplers)                           3 + 1 = K_XS       4
    DDPM x_next       x_start 3, 2 products, 1 add; with noise 1 product, 1 add more,
                      and expf at EXPF_ULPS ulps = 2 EXPF_ULPS units of 2^-24              6 + 1 = 7; 8 + 2 EXPF_ULPS + 1 = K_DDPM_NOISE 13
    DDIM x_next       a 1, x_start 2 more, a - st 1, / c2 1, 3 products, 2 adds            10 + 1 = K_DDIM    11   (noise == NULL: x_start, K_XS)
    fused gradient    out - tgt 1, wc wb 1, 2 df exact, (2 df) wgt 1, inv_count 1          4 + 1 = K_GRAD     5
    backward          out - tgt 1, wc wb 1, df wgt 1, gs = (2 inv_count) gscale 1, gs 1    5 + 1 = K_BWD      6
    loss              per term: df enters squared 2, the square 1, wc wb 1; the cast 1     5 + 1 = K_LOSS     6    (the sum and the scaling run in
                      fp64: n 2^-53 relative to the sum of |terms|, below 1e-9 units for n <= 4e6)
EXPF_ULPS: ROCm publishes a maximum error in ulps for the device expf in the HIP math API reference; the installed toolchain carries no copy of it, so 2 is
an ASSUMPTION (one ulp is at most two units of 2^-24). The clamp: S of x_start is |c1 x| + |c2 eps| where the unclamped fp64 value lies within
K_XS 2^-24 S of [-1, 1] (a correct fp32 value may land on either side of the bound) and 0 -- the result must be exactly -1 or 1 -- beyond it;
downstream the scale of x_start is that S where near, and 1 where far. For DDIM this makes S_e include (|c1 x| + S(x_start)) / c2 for the
re-derived noise: at small c2 the reference's own fp32 arithmetic loses the same bits. Where S_e = 0 the result must equal the reference exactly.
Exact bits: code 2 -> the source's bits, code 1 -> +0, the target the noise's bits or +0, untouched elements of apply_cond keep their bits,
clamped x_start in [-1, 1], DDIM-dev == DDIM with the same scalars.

CASES. Every case names the regime it exists for and states the form and the grid the plan query must report; REQUIRED is what the matrix as a
whole must reach (check_coverage)."""
import itertools

import numpy as np
import torch

from oracle import diffusion_ref as D

U = 2.0 ** -24
EXPF_ULPS = 2
K_Q, K_XS, K_DDPM, K_DDIM, K_GRAD, K_BWD, K_LOSS = 4, 4, 7, 11, 5, 6, 6
K_DDPM_NOISE = 8 + 2 * EXPF_ULPS + 1
SENTINEL = -7.25                       # guard bands
UNWRITTEN = 0x7FC00ABC                 # bit pattern (a NaN no arithmetic produces) an output holds before the launch
GUARD = 64                             # floats before and after every operand
WDNO_EINVAL, WDNO_EWORKSPACE = -1, -4


# ------------------------------------------------------------------------------------------------------------------ three arithmetics
class Arith:
    def __init__(self, dtype, fused=False):
        self.dt, self.fused = np.dtype(dtype), fused

    def c(self, v):
        """an fp32 input value in this arithmetic (exact)"""
        return np.asarray(v, np.float32).astype(self.dt)

    def muladd(self, a, b, c):
        """a b + c: two roundings, or one where the compiler contracts. The fused form is the fp64 value rounded to fp32: the product of two
        fp32 numbers is exact in fp64, so only the double rounding of the sum separates it from a hardware fma (one case in 2^29)."""
        if self.fused and self.dt == np.float32:
            return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
        return a * b + c


F64, F32, F32FMA = Arith(np.float64), Arith(np.float32), Arith(np.float32, fused=True)


def _per_sample(table, t, ndim):
    return np.asarray(table)[np.asarray(t)].reshape((-1,) + (1,) * (ndim - 1))


# ------------------------------------------------------------------------------------------------------------------ masks
SMOKE_FLAGS = ('pad', 'control', 'low')
BURGERS_FLAGS = ('pad', 'u0', 'uT', 'f', 'low')


def oracle_codes(c):
    """[1, ...] int code per element (0 free, 1 zero, 2 clean) from the oracle's in-place statements on marker tensors"""
    fl = c['flags']
    shape = (1,) + tuple(c['shape'][1:])
    img = torch.full(shape, 7.0, dtype=torch.float64)
    if c['tree'] == 0:
        D.smoke_apply_conditions(img, c['coef'], init=2.0, control=2.0, low=2.0, is_condition_control=fl['control'], is_condition_pad=fl['pad'],
                                 is_super_model=fl['low'])
    else:
        _, C, H, W = shape
        two = lambda *s: torch.full(s, 2.0, dtype=torch.float64)
        D.burgers_apply_conditions(img, c['coef'], fl, u0=two(1, c['u_rows'], W), uT=two(1, c['uT_rows'], W), f=two(1, 4, H, W),
                                   low=two(1, max(min(16, C) - 8, 0), H, W))
    code = np.zeros(shape, np.int8)
    a = img.numpy()
    assert np.isin(a, (7.0, 0.0, 2.0)).all()
    code[a == 0.0] = 1
    code[a == 2.0] = 2
    return code


def smoke_rules(c):
    """(name, value, predicate) of diffusion_2d.py:1008-1033 in statement order"""
    _, F, C, H, W = c['shape']
    cT, cH, cW = c['coef']
    f, ch, h, w = np.meshgrid(np.arange(F), np.arange(C), np.arange(H), np.arange(W), indexing='ij')
    fl = c['flags']
    no = np.zeros_like(f, bool)
    return [('init', 2, ch == C - 2),
            ('control', 2, (ch >= 24) & (ch < 40) if fl['control'] else no),
            ('pad', 1, ((f >= cT) & (ch != C - 2)) | ((ch != C - 1) & ((h >= cH) | (w >= cW))) if fl['pad'] else no),
            ('low', 2, (ch >= 40) & (ch < 80) if fl['low'] else no)]


def burgers_rules(c):
    """diffusion_1d.py:276-288 in call order pad, u0, uT, f, low"""
    _, C, H, W = c['shape']
    cH, cW = c['coef']
    ch, h, w = np.meshgrid(np.arange(C), np.arange(H), np.arange(W), indexing='ij')
    fl = c['flags']
    no = np.zeros_like(ch, bool)
    inside = (h < cH) & (w < cW)
    return [('pad', 1, ((ch != C - 1) & (h >= cH)) | (w >= cW) if fl['pad'] else no),
            ('u0', 2, (ch == C - 1) & (h < c['u_rows']) & (w < cW) if fl['u0'] else no),
            ('uT', 2, (ch == C - 1) & (h >= H - c['uT_rows']) & (w < cW) if fl['uT'] else no),
            ('f', 2, (ch >= 4) & (ch < 8) & inside if fl['f'] else no),
            ('low', 2, (ch >= 8) & (ch < 16) & inside if fl['low'] else no)]


def cond_table(c, swap=None):
    """the code of every element chosen per element: the LAST statement whose predicate holds. swap = (name, name): those two statements
    trade places (a planted fault)"""
    rules = smoke_rules(c) if c['tree'] == 0 else burgers_rules(c)
    if swap:
        i, j = (next(k for k, r in enumerate(rules) if r[0] == n) for n in swap)
        rules[i], rules[j] = rules[j], rules[i]
    rules = rules[::-1]
    return np.select([r[2] for r in rules], [r[1] for r in rules], 0).astype(np.int8)[None]


# ------------------------------------------------------------------------------------------------------------------ formulas
def q_sample(ar, x0, noise, t, sa, sb, t_shift=0):
    tt = np.roll(np.asarray(t), t_shift)
    ka, kb = ar.c(_per_sample(sa, tt, x0.ndim)), ar.c(_per_sample(sb, tt, x0.ndim))
    return ar.muladd(ka, ar.c(x0), kb * ar.c(noise))


def q_sample_scale(x0, noise, t, sa, sb):
    ka, kb = F64.c(_per_sample(sa, t, x0.ndim)), F64.c(_per_sample(sb, t, x0.ndim))
    return np.abs(ka * F64.c(x0)) + np.abs(kb * F64.c(noise))


def cond_reference(c, x0, noise, t, sa, sb, code=None):
    """dict(code, x, x_scale, target): x exact (scale 0) wherever the code is not 0; target exact everywhere"""
    code = np.broadcast_to(oracle_codes(c) if code is None else code, x0.shape)
    x = np.where(code == 0, q_sample(F64, x0, noise, t, sa, sb), np.where(code == 1, 0.0, F64.c(x0)))
    return dict(code=code, x=x, x_scale=np.where(code == 0, q_sample_scale(x0, noise, t, sa, sb), 0.0), target=np.where(code == 0, noise, np.float32(0)))


def cond_transcription(ar, c, x0, noise, t, sa, sb, code=None, t_shift=0):
    code = np.broadcast_to(oracle_codes(c) if code is None else code, x0.shape)
    x = np.where(code == 0, q_sample(ar, x0, noise, t, sa, sb, t_shift), np.where(code == 1, np.float32(0), x0))
    return x, np.where(code == 0, noise, np.float32(0))


def apply_reference(c, x, src, code=None):
    code = np.broadcast_to(oracle_codes(c) if code is None else code, x.shape)
    return np.where(code == 0, x, np.where(code == 1, np.float32(0), src))


def _weights(ar, wc, wb, B, F, C, inner, chan_without_f=False):
    """[B, F C inner] weight wc[c(e)] wb[b(e)], one product. chan_without_f: the channel taken as e / (F inner) (a planted fault)"""
    e = np.arange(F * C * inner)
    ch = (e // (inner * F)) % C if chan_without_f else (e // inner) % C
    return ar.c(wc)[ch][None, :] * ar.c(wb)[:, None]


def loss_terms(ar, out, tgt, wc, wb, F, C, inner, **fault):
    """(df, wgt, df^2) over [B, F C inner]"""
    B = out.shape[0]
    df = ar.c(out).reshape(B, -1) - ar.c(tgt).reshape(B, -1)
    return df, _weights(ar, wc, wb, B, F, C, inner, **fault), df * df


def loss_value(ar, out, tgt, wc, wb, inv, F, C, inner, **fault):
    """fp32 squares and weights, fp64 sum (as the issue states the loss), the result in the arithmetic's dtype"""
    df, wgt, sq = loss_terms(ar, out, tgt, wc, wb, F, C, inner, **fault)
    return ar.dt.type((sq.astype(np.float64) * wgt.astype(np.float64)).sum() * np.float64(np.float32(inv)))


def loss_scale(out, tgt, wc, wb, inv, F, C, inner):
    B = out.shape[0]
    s = np.abs(F64.c(out).reshape(B, -1)) + np.abs(F64.c(tgt).reshape(B, -1))
    return float((s * s * np.abs(_weights(F64, wc, wb, B, F, C, inner))).sum() * np.float64(np.float32(inv)))


def loss_grad(ar, out, tgt, wc, wb, inv, F, C, inner, gscale=None, fused_arm=False, **fault):
    """fused_arm: ((2 df) wgt) inv_count as the forward writes it; else (df wgt) ((2 inv_count) gscale)"""
    df, wgt, _ = loss_terms(ar, out, tgt, wc, wb, F, C, inner, **fault)
    two, k = ar.dt.type(2), ar.c(inv)
    if fused_arm:
        return ((two * df) * wgt * k).reshape(out.shape)
    gs = two * k * (ar.c(gscale) if gscale is not None else ar.dt.type(1))
    return ((df * wgt) * gs).reshape(out.shape)


def loss_grad_scale(out, tgt, wc, wb, inv, F, C, inner, gscale=None):
    B = out.shape[0]
    s = np.abs(F64.c(out).reshape(B, -1)) + np.abs(F64.c(tgt).reshape(B, -1))
    g = abs(float(np.float32(gscale))) if gscale is not None else 1.0
    return (2.0 * s * np.abs(_weights(F64, wc, wb, B, F, C, inner)) * float(np.float32(inv)) * g).reshape(out.shape)


def x_start(ar, x, eps, t, c1, c2, clamp=True, t_shift=0):
    """(a, st): a = c1 x, st = clamp(a - c2 eps)"""
    tt = np.roll(np.asarray(t), t_shift)
    k1, k2 = ar.c(_per_sample(c1, tt, x.ndim)), ar.c(_per_sample(c2, tt, x.ndim))
    a = k1 * ar.c(x)
    st = ar.muladd(-k2, ar.c(eps), a)
    return a, (np.clip(st, ar.dt.type(-1), ar.dt.type(1)) if clamp else st)


def x_start_scale(x, eps, t, c1, c2, clamp=True):
    """(S of x_start as an output, S of x_start as an operand downstream)"""
    k1, k2 = F64.c(_per_sample(c1, t, x.ndim)), F64.c(_per_sample(c2, t, x.ndim))
    s = np.abs(k1 * F64.c(x)) + np.abs(k2 * F64.c(eps))
    if not clamp:
        return s, s
    _, raw = x_start(F64, x, eps, t, c1, c2, clamp=False)
    near = np.abs(raw) <= 1.0 + K_XS * U * s
    return np.where(near, s, 0.0), np.where(near, s, 1.0)


def ddpm_update(ar, x, eps, noise, t, tab, clamp=True, **fault):
    """tab = (c1, c2, m1, m2, lv) -> (x_next, x_start). exp is evaluated in fp64 and rounded to the arithmetic's dtype (a correctly rounded expf)"""
    c1, c2, m1, m2, lv = tab
    _, st = x_start(ar, x, eps, t, c1, c2, clamp, **fault)
    q1, q2 = ar.c(_per_sample(m1, t, x.ndim)), ar.c(_per_sample(m2, t, x.ndim))
    mean = ar.muladd(q1, st, q2 * ar.c(x))
    if noise is None:
        return mean, st
    sg = np.exp(0.5 * F64.c(_per_sample(lv, t, x.ndim))).astype(ar.dt)
    return ar.muladd(sg, ar.c(noise), mean), st


def ddpm_scale(x, eps, noise, t, tab, clamp=True):
    c1, c2, m1, m2, lv = tab
    s_out, s_op = x_start_scale(x, eps, t, c1, c2, clamp)
    q1, q2 = F64.c(_per_sample(m1, t, x.ndim)), F64.c(_per_sample(m2, t, x.ndim))
    s = np.abs(q1) * s_op + np.abs(q2 * F64.c(x))
    if noise is not None:
        s = s + np.exp(0.5 * F64.c(_per_sample(lv, t, x.ndim))) * np.abs(F64.c(noise))
    return s, s_out


def ddim_update(ar, x, eps, noise, t, tab, coef, clamp=True, **fault):
    """tab = (c1, c2), coef = (sqrt_an, c, sigma) -> (x_next, x_start); the update always clamps (clamp = False is a planted fault)"""
    c1, c2 = tab[:2]
    a, st = x_start(ar, x, eps, t, c1, c2, clamp, **fault)
    if noise is None:
        return st, st
    k2 = ar.c(_per_sample(c2, t, x.ndim))
    san, cc, sigma = (ar.c(v) for v in coef)
    e2 = (a - st) / k2
    return ar.muladd(sigma, ar.c(noise), ar.muladd(cc, e2, st * san)), st


def ddim_scale(x, eps, noise, t, tab, coef):
    c1, c2 = tab[:2]
    s_out, s_op = x_start_scale(x, eps, t, c1, c2, True)
    if noise is None:
        return s_out, s_out
    k1, k2 = F64.c(_per_sample(c1, t, x.ndim)), F64.c(_per_sample(c2, t, x.ndim))
    san, cc, sigma = (abs(float(np.float32(v))) for v in coef)
    return s_op * san + cc * (np.abs(k1 * F64.c(x)) + s_op) / np.abs(k2) + sigma * np.abs(F64.c(noise)), s_out


def ratio(got, ref, scale):
    """max over the elements of |got - ref| / (2^-24 S_e); inf where S_e = 0 and got != ref, or got is not finite"""
    got = np.asarray(got, np.float64)
    ref, scale = np.broadcast_to(ref, got.shape), np.broadcast_to(scale, got.shape)
    if not np.isfinite(got).all() or ((scale == 0) & (got != ref)).any():
        return float('inf')
    nz = scale > 0
    return float((np.abs(got - ref)[nz] / (U * scale[nz])).max()) if nz.any() else 0.0


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------------------------ inputs
T_STEPS = 1000
_BUF = {}


def tables(kind):
    """the fp32 schedule buffers of the oracle as numpy arrays"""
    if kind not in _BUF:
        _BUF[kind] = {k: v.numpy() for k, v in D.make_buffers(kind, T_STEPS).items()}
    return _BUF[kind]


def update_tables(kind='linear'):
    b = tables(kind)
    return tuple(b[k] for k in ('sqrt_recip_alphas_cumprod', 'sqrt_recipm1_alphas_cumprod', 'posterior_mean_coef1', 'posterior_mean_coef2',
                                'posterior_log_variance_clipped'))


def ddim_coef():
    """(sqrt_an, c, sigma) of one DDIM step of the linear schedule, fp32 values"""
    sigma, c, san = D.ddim_scalars(D.make_buffers('linear', T_STEPS), 600, 300, 0.7)
    return tuple(float(np.float32(v)) for v in (san, c, sigma))


def seed_of(name):
    """deterministic across processes (hash() of a str is not)"""
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % (2 ** 31)


def sample_t(B):
    """per-sample timesteps that include 0 and T - 1"""
    t = np.array([0, T_STEPS - 1, 3, 500, 977, 41, 250], np.int64)
    return np.resize(t, B)


def cond_inputs(c):
    rng = np.random.default_rng(seed_of(c['name']))
    shape = c['shape']
    return dict(x0=rng.standard_normal(shape).astype(np.float32), noise=rng.standard_normal(shape).astype(np.float32), t=sample_t(shape[0]),
                x=rng.standard_normal(shape).astype(np.float32))


def loss_inputs(c):
    rng = np.random.default_rng(seed_of(c['name']))
    shape = (c['B'], c['F'], c['C'], c['inner'])
    return dict(out=rng.standard_normal(shape).astype(np.float32), tgt=rng.standard_normal(shape).astype(np.float32),
                wc=(0.5 + 0.37 * np.arange(c['C'])).astype(np.float32), wb=(1.0 + 0.0625 * (np.arange(c['B']) % 29) + 0.001 * (np.arange(c['B']) % 7)).astype(np.float32),
                inv=np.float32(1.0 / (c['B'] * c['F'] * c['C'] * c['inner'])), gscale=np.float32(0.731))


def update_inputs(c):
    """x, eps scaled so that x_start clamps on both sides and stays free in between for the early timesteps"""
    rng = np.random.default_rng(seed_of(c['name']))
    shape = (c['B'], c['per_sample'])
    return dict(x=(0.9 * rng.standard_normal(shape)).astype(np.float32), eps=rng.standard_normal(shape).astype(np.float32),
                noise=rng.standard_normal(shape).astype(np.float32), t=sample_t(c['B']))


# ------------------------------------------------------------------------------------------------------------------ the case matrix
def grid1(n):
    """blocks of 256 threads over n work items, capped at 2048"""
    return max(1, min(2048, -(-n // 256)))


def rounds(n, blocks):
    """(grid-stride rounds the busiest thread takes, whether the last one is ragged)"""
    return -(-n // (blocks * 256)), n % (blocks * 256) != 0


COND_CASES, LOSS_CASES, UPDATE_CASES = [], [], []
COND_OPERANDS = ('x0', 'noise', 'x', 'target')          # apply_cond: x0 / x misalign its x, noise / target its src


def _cond(name, regime, tree, shape, coef, flags, form, misalign=None, u_rows=0, uT_rows=0, plain=False):
    total = int(np.prod(shape))
    expect = (form, grid1(total // 4 if form == 'float4' else total), 1)
    names = SMOKE_FLAGS if tree == 0 else BURGERS_FLAGS
    COND_CASES.append(dict(name=name, regime=regime, tree=tree, shape=tuple(shape), coef=tuple(coef), flags=dict(zip(names, flags)), expect=expect,
                           misalign=misalign, u_rows=u_rows, uT_rows=uT_rows, plain=plain, total=total))


def _flagname(names, flags):
    return '+'.join(n for n, f in zip(names, flags) if f) or 'none'


# smoke: [2, 3, C, 6, 8] with coefficient extents (2, 5, 6): frame 2 beyond cT, row 5 beyond cH, the float4 group w = 4 .. 7 straddles cW = 6
for _fl in itertools.product((False, True), repeat=3):
    for _C in (42, 82) if _fl[2] else (42,):
        _n = f'C{_C}-{_flagname(SMOKE_FLAGS, _fl)}'
        _cond(f'smoke-w8-{_n}', 'smoke masks, float4', 0, (2, 3, _C, 6, 8), (2, 5, 6), _fl, 'float4')
        _cond(f'smoke-w6-{_n}', 'smoke masks, scalar by W % 4', 0, (2, 3, _C, 6, 6), (2, 5, 5), _fl, 'scalar')
for _op in COND_OPERANDS:
    _cond(f'smoke-w8-misaligned-{_op}', f'smoke masks, scalar by a 4-byte offset of {_op}', 0, (2, 3, 82, 6, 8), (2, 5, 6), (True, True, True), 'scalar',
          misalign=_op)
# Burgers: [2, C, 16, 12] with (11, 10): the uT rows 8 .. 15 reach into the padded rows 11 .. 15, the u0 rows 0 .. 8 meet them at row 8, the group
# w = 8 .. 11 straddles cW = 10; and W = 14 (not a multiple of 4)
for _fl in itertools.product((False, True), repeat=5):
    for _C in (9, 17) if _fl[4] else (9,):
        _n = f'C{_C}-{_flagname(BURGERS_FLAGS, _fl)}'
        _cond(f'burgers-w12-{_n}', 'Burgers masks, float4', 1, (2, _C, 16, 12), (11, 10), _fl, 'float4', u_rows=9, uT_rows=8)
        _cond(f'burgers-w14-{_n}', 'Burgers masks, scalar by W % 4', 1, (2, _C, 16, 14), (11, 10), _fl, 'scalar', u_rows=9, uT_rows=8)
_cond('plain', 'plain_desc: no conditioning, the sample as one row', 1, (3, 1, 1, 40), (1, 40), (False,) * 5, 'float4', plain=True)
_cond('plain-odd', 'plain_desc, scalar by an odd row', 1, (3, 1, 1, 37), (1, 37), (False,) * 5, 'scalar', plain=True)
# more work items than 2048 x 256 = 524 288: a second, ragged round. 2 116 800 elements = 529 200 float4; 529 200 elements
_cond('rounds-float4', 'float4, 529 200 work items on 2048 blocks: second round of 4 912', 1, (3, 9, 100, 784), (90, 700), (True,) * 5, 'float4', u_rows=50,
      uT_rows=50)
_cond('rounds-scalar', 'scalar, 529 200 work items on 2048 blocks: second round of 4 912', 1, (2, 9, 100, 294), (90, 250), (True,) * 5, 'scalar', u_rows=50,
      uT_rows=50)
COND_BY_NAME = {c['name']: c for c in COND_CASES}
assert len(COND_BY_NAME) == len(COND_CASES)

LOSS_OPERANDS = ('out', 'tgt', 'grad')


def _loss(name, regime, B, F, C, inner, fwd, bwd, misalign=None):
    """fwd / bwd: (form, grid_x, grid_y) the plan query must report for the forward (with or without the gradient) and the backward"""
    LOSS_CASES.append(dict(name=name, regime=regime, B=B, F=F, C=C, inner=inner, per_sample=F * C * inner, fwd=fwd, bwd=bwd, misalign=misalign))


_loss('float4', 'float4: 3 samples of 2 x 5 x 52 = 130 float4', 3, 2, 5, 52, ('float4', 1, 3), ('float4', 1, 3))
_loss('float4-blocks', 'float4, three blocks per sample, the last ragged', 3, 2, 5, 264, ('float4', 3, 3), ('float4', 3, 3))
_loss('scalar-inner', 'scalar by inner % 4 != 0', 3, 2, 5, 54, ('scalar', 7, 1), ('scalar', 7, 1))
for _op in LOSS_OPERANDS:
    _loss(f'scalar-misaligned-{_op}', f'scalar by a 4-byte offset of {_op}', 3, 2, 5, 52, ('scalar', 7, 1), ('scalar', 7, 1), misalign=_op)
_loss('scalar-nb', 'forward scalar by nb = 75 < B = 300 (per_sample 64); the backward stays float4', 300, 2, 2, 16, ('scalar', 75, 1), ('float4', 1, 300))
_loss('scalar-B', 'scalar by B = 2049 > 2048, forward and backward', 2049, 2, 2, 4, ('scalar', 129, 1), ('scalar', 129, 1))
_loss('rounds-float4', 'float4, 132 000 float4 per sample on 512 blocks: second round of 928, forward and backward', 4, 2, 3, 88000, ('float4', 512, 4),
      ('float4', 512, 4))
LOSS_BY_NAME = {c['name']: c for c in LOSS_CASES}

UPDATE_OPERANDS = ('x', 'eps', 'noise', 'x_next', 'x_start')


def _upd(name, regime, B, per_sample, expect, misalign=None):
    UPDATE_CASES.append(dict(name=name, regime=regime, B=B, per_sample=per_sample, expect=expect, misalign=misalign))


_upd('float4', 'float4: 3 samples of 1 300 (325 float4: two blocks, the second ragged)', 3, 1300, ('float4', 2, 3))
_upd('scalar-odd', 'scalar by per_sample % 4 != 0', 3, 1301, ('scalar', 16, 1))
for _op in UPDATE_OPERANDS:
    _upd(f'scalar-misaligned-{_op}', f'scalar by a 4-byte offset of {_op}', 3, 1300, ('scalar', 16, 1), misalign=_op)
_upd('scalar-B', 'scalar by B = 65 536 > 65 535 with per_sample 4', 65536, 4, ('scalar', 1024, 1))
_upd('rounds-float4', 'float4, 175 000 float4 per sample on 683 blocks: second round of 152', 3, 700000, ('float4', 683, 3))
UPDATE_BY_NAME = {c['name']: c for c in UPDATE_CASES}


def cond_desc_of(K, c):
    """the descriptor of a case through the library's own constructors (wdno_amd.diffusion_core)"""
    fl = c['flags']
    if c['plain']:
        return K.plain_desc(torch.empty(c['shape']))
    if c['tree'] == 0:
        return K.cond_desc(0, c['shape'], c['coef'], fl['pad'], fl['control'], 0, 0, fl['low'])
    return K.cond_desc(1, c['shape'], c['coef'], fl['pad'], fl['u0'], fl['uT'], fl['f'], fl['low'], c['u_rows'], c['uT_rows'])


def plan_tuple(p):
    return (p['form'], p['grid_x'], p['grid_y'])


def cond_plans(K, c):
    """{'q': plan of q_sample_cond, 'a': plan of apply_cond} for the alignment the case asks for"""
    m = 4 if c['misalign'] else 0
    return {'q': K.cond_plan(cond_desc_of(K, c), m), 'a': K.cond_plan(cond_desc_of(K, c), m)}


def loss_plans(K, c):
    """'fwd' (no gradient; a misaligned grad is no operand of it), 'fwd_grad', 'bwd'"""
    m = 4 if c['misalign'] else 0
    arg = (c['B'], c['per_sample'], c['C'], c['inner'])
    return {'fwd': K.weighted_mse_plan(*arg, align_mask=0 if c['misalign'] == 'grad' else m), 'fwd_grad': K.weighted_mse_plan(*arg, align_mask=m),
            'bwd': K.weighted_mse_plan(*arg, backward=True, align_mask=m)}


def loss_expect(c, arm):
    if arm == 'fwd' and c['misalign'] == 'grad':
        return LOSS_BY_NAME['float4']['fwd']
    return c['bwd'] if arm == 'bwd' else c['fwd']


def update_plan(K, c, arm_operands=UPDATE_OPERANDS):
    """the plan of one update launch; arm_operands: the operands the arm passes (a NULL noise or x_start cannot be misaligned)"""
    m = 4 if c['misalign'] in arm_operands else 0
    return K.update_plan(c['B'], c['per_sample'], m)


def update_expect(c, arm_operands=UPDATE_OPERANDS):
    if c['misalign'] and c['misalign'] not in arm_operands:
        return UPDATE_BY_NAME['float4']['expect']
    return c['expect']


# ------------------------------------------------------------------------------------------------------------------ coverage
# (kernel, arm): every kernel of the unit in every arm the launch code can put it in
REQUIRED = {
    ('q_sample_cond4_kernel', 'smoke'), ('q_sample_cond4_kernel', 'burgers'), ('q_sample_cond4_kernel', 'plain'), ('q_sample_cond4_kernel', 'rounds'),
    ('q_sample_cond_kernel', 'smoke'), ('q_sample_cond_kernel', 'burgers'), ('q_sample_cond_kernel', 'plain'), ('q_sample_cond_kernel', 'rounds'),
    ('q_sample_cond_kernel', 'misaligned'),
    ('apply_cond4_kernel', 'smoke'), ('apply_cond4_kernel', 'burgers'), ('apply_cond4_kernel', 'rounds'),
    ('apply_cond_kernel', 'smoke'), ('apply_cond_kernel', 'burgers'), ('apply_cond_kernel', 'rounds'), ('apply_cond_kernel', 'misaligned'),
    ('wmse4_kernel<false>', 'loss'), ('wmse4_kernel<false>', 'grad'), ('wmse4_kernel<false>', 'rounds'),
    ('wmse_kernel', 'loss'), ('wmse_kernel', 'grad'), ('wmse_kernel', 'inner'), ('wmse_kernel', 'misaligned'), ('wmse_kernel', 'nb<B'), ('wmse_kernel', 'B>2048'),
    ('wmse_final_kernel', 'float4'), ('wmse_final_kernel', 'scalar'),
    ('wmse4_kernel<true>', 'gscale'), ('wmse4_kernel<true>', 'no-gscale'), ('wmse4_kernel<true>', 'rounds'),
    ('wmse_bwd_kernel', 'gscale'), ('wmse_bwd_kernel', 'no-gscale'), ('wmse_bwd_kernel', 'inner'), ('wmse_bwd_kernel', 'misaligned'), ('wmse_bwd_kernel', 'B>2048'),
} | {(k, arm) for k in ('p_sample4_kernel', 'ddim4_kernel') for arm in ('noise', 'no-noise', 'no-x_start', 'rounds')} \
  | {(k, arm) for k in ('p_sample_kernel', 'ddim_kernel') for arm in ('noise', 'no-noise', 'no-x_start', 'odd', 'misaligned', 'B>65535')} \
  | {('p_sample4_kernel', 'clamp-off'), ('p_sample_kernel', 'clamp-off'), ('ddim4_kernel', 'dev'), ('ddim_kernel', 'dev')}
KERNELS = {'q_sample_cond_kernel', 'q_sample_cond4_kernel', 'apply_cond_kernel', 'apply_cond4_kernel', 'wmse_kernel', 'wmse_final_kernel', 'wmse4_kernel<false>',
           'wmse4_kernel<true>', 'wmse_bwd_kernel', 'p_sample_kernel', 'p_sample4_kernel', 'ddim_kernel', 'ddim4_kernel'}

# the arms every update case runs (tests/test_gpu_diffusion_matrix.py::test_update_gate): name -> (kernel family, operands passed)
UPDATE_ARMS = {
    'ddpm': ('p_sample', UPDATE_OPERANDS, 'noise'), 'ddpm-no-noise': ('p_sample', ('x', 'eps', 'x_next', 'x_start'), 'no-noise'),
    'ddpm-no-x_start': ('p_sample', ('x', 'eps', 'noise', 'x_next'), 'no-x_start'), 'ddpm-clamp-off': ('p_sample', UPDATE_OPERANDS, 'clamp-off'),
    'ddim': ('ddim', UPDATE_OPERANDS, 'noise'), 'ddim-no-noise': ('ddim', ('x', 'eps', 'x_next', 'x_start'), 'no-noise'),
    'ddim-no-x_start': ('ddim', ('x', 'eps', 'noise', 'x_next'), 'no-x_start'), 'ddim-dev': ('ddim', UPDATE_OPERANDS, 'dev'),
}


def _regime_arm(c):
    n = c['name']
    if n.startswith('rounds'):
        return 'rounds'
    if 'misaligned' in n:
        return 'misaligned'
    for key, arm in (('scalar-inner', 'inner'), ('scalar-nb', 'nb<B'), ('scalar-B', 'B>2048'), ('scalar-odd', 'odd')):
        if n.startswith(key):
            return arm
    return None


def check_coverage(K):
    """REQUIRED, computed from the plans of the cases and the arms the GPU test runs on each; every kernel of the unit is named in it. A 'rounds'
    arm counts only where the plan's grid leaves a second, ragged round. Returns a line that says what was reached."""
    seen = set()
    for c in COND_CASES:
        for which, p in cond_plans(K, c).items():
            assert p['rc'] == 0, (c['name'], p)
            kern = {'q': 'q_sample_cond', 'a': 'apply_cond'}[which] + ('4_kernel' if p['form'] == 'float4' else '_kernel')
            n = c['total'] // 4 if p['form'] == 'float4' else c['total']
            arm = _regime_arm(c) or ('plain' if c['plain'] else ('smoke', 'burgers')[c['tree']])
            if arm == 'rounds' and rounds(n, p['grid_x']) != (2, True):
                continue
            if not (c['plain'] and which == 'a'):
                seen.add((kern, arm))
    for c in LOSS_CASES:
        for arm_name, p in loss_plans(K, c).items():
            assert p['rc'] == 0, (c['name'], p)
            f4 = p['form'] == 'float4'
            n = c['per_sample'] // 4 if f4 else c['B'] * c['per_sample']
            second = rounds(n, p['grid_x']) == (2, True)
            special = _regime_arm(c)
            if special == 'B>2048' and (f4 or c['B'] <= 2048):
                special = None
            if arm_name == 'bwd':
                kern = 'wmse4_kernel<true>' if f4 else 'wmse_bwd_kernel'
                arms = {'gscale', 'no-gscale'}
            else:
                kern = 'wmse4_kernel<false>' if f4 else 'wmse_kernel'
                arms = {'loss' if arm_name == 'fwd' else 'grad'}
                seen.add(('wmse_final_kernel', p['form']))
            if special == 'rounds':
                arms = {'rounds'} if second else set()
            elif special and not f4:
                arms.add(special)
            seen |= {(kern, a) for a in arms}
    for c in UPDATE_CASES:
        for fam, operands, arm in UPDATE_ARMS.values():
            p = update_plan(K, c, operands)
            assert p['rc'] == 0, (c['name'], p)
            f4 = p['form'] == 'float4'
            kern = fam + ('4_kernel' if f4 else '_kernel')
            seen.add((kern, arm))
            special = _regime_arm(c)
            if special == 'B>2048':
                special = 'B>65535'
            n = c['per_sample'] // 4 if f4 else c['B'] * c['per_sample']
            if special == 'rounds':
                if rounds(n, p['grid_x']) == (2, True):
                    seen.add((kern, 'rounds'))
            elif special and not f4:
                seen.add((kern, special))
    assert {k for k, _ in REQUIRED} == KERNELS and len(KERNELS) == 13
    missing = sorted(REQUIRED - seen)
    assert not missing, missing
    return f'reached {len(REQUIRED)} of {len(REQUIRED)} required (kernel, arm) pairs over {len(KERNELS)} kernels; ' \
           f'{len(COND_CASES)} condition, {len(LOSS_CASES)} loss and {len(UPDATE_CASES)} update cases'
