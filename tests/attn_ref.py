"""The two fused attention blocks in plain torch on the CPU, fp64, forward and hand-written backward (no autograd), with an ERROR SCALE and a
FLUSH term for every output. Test infrastructure only. The operations are the ones the kernel headers state:

  temporal (csrc/attn_fused.hip, attn_fused48.hip, attn_fused_wide.hip, attn_fused_bwd.hip), per sequence = the F frames of one pixel:
      y = x + W_out softmax(rot(scale q) rot(k)^T + bias) v          (q | k | v) = W_qkv LayerNorm(x)
  linear (csrc/linattn_fused.hip, linattn_fused_wide.hip, linattn_fused_bwd.hip), per unit = one frame of n = H W tokens, and head:
      y = x + b_out + W_out out      out[n][e] = sum_d ctx[d][e] qs[n][d]      ctx[d][e] = sum_n ks[n][d] v[n][e]
      qs = scale softmax_d(q)        ks = softmax_n(k)                          (q | k | v) = W_qkv LayerNorm(x)

checked against oracle/unet_ref.py (channel_layernorm + token_attention / linear_attention_2d) and its autograd by
tests/test_host_attn_ref.py. Tensors are channels-last [B, F, H, W, C] as the library sees them.

THE GATE is element-wise:  |got - ref| <= K 2^-24 scale + flush.  `scale` is the same formula evaluated on the absolute values of the terms
the kernels add, carried stage by stage (first order: the error of each factor times the size of the other), so a result that cancels is
held to the rounding of its terms and not to its own size:

    xs (LayerNorm)  = (|x| + |mean|) rstd |gamma|                    (as tests/groupnorm_ref.py's xs; >= |xn|)
    projection      = xs |W_qkv|^T                                   rotary: |cos| s_x + |sin| s_y; q also times the softmax scale
    logits          = s_q |k|^T + |q| s_k^T + |bias|
    softmax         = p (1 + s_l + sum p s_l)                        the ABSOLUTE error scale of the logits enters p as a RELATIVE error
                                                                     (d p_i = p_i (d l_i - sum_j p_j d l_j)), the 1 is p's own rounding
    products        = s_a |b| + |a| s_b                              context, output, to_out; the residual adds |y|
    backward        = the same stages in reverse; (dp - delta), (dqs - inner), (dks - T) enter as |dp| + |delta|, ...; LayerNorm backward as
                      groupnorm_ref's dx: rstd (s_dn + mean s_dn + |xh| s_m2 + xs_h |m2|) + |dxl|

Flush terms, after tests/conv_ref.py: a `lo` plane entry below 2^-14 in scaled units is a sub-normal fp16 and carries an absolute error of
2^-25 / s <= 2^-39 amax; per product of two plane tensors that is 2^-40 (amax(a) sum |b| + amax(b) sum |a|). They are carried through the
later stages like the scales. The backward kernels keep RUNNING plane scales for dq / dk / dv (and the linear backward for out): a tile is
split at the scale of the largest tile its wave has met so far. That maximum never exceeds the tensor's global maximum, a plane scale only
shrinks as its amax grows, and the sub-normal error 2^-25 / s grows as s shrinks: so the flush computed from the reference's global
max|.| of the tensor bounds the flush of every tile, whichever block and order met it.

K, one per output kind (linear attention: y, dx and the weight gradients also per reduction-length class, `short` below LONG = 1024 tokens per
frame and `long` from it on: the context sums n_tok terms in fp32), is NOT taken from the kernels. transcription_t / transcription_l restate the
kernels' arithmetic in fp32 torch: two-pass LayerNorm, (hi, lo) fp16 planes at the kernels' power-of-two scales and the three plane products
hi lo + lo hi + hi hi for everything the kernels run on the split matrix instruction, plain fp32 for what they run on the exact-fp32 one, the
online softmax over token chunks with its merge for linear attention. The worst ratio over the whole matrix (tests/test_host_attn_ref.py
re-measures it and holds it to K / 2) is

    MEASURED = {t_y: 0.018, t_dx: 0.034, t_dw: 0.021, t_dgamma: 0.0003, t_dbias: 0.141,
                l_y_short: 0.122, l_y_long: 0.164, l_dx_short: 0.028, l_dx_long: 0.022, l_dw_short: 0.119, l_dw_long: 0.007, l_dgamma: 0.002,
                l_db_out: 1.328}

(far below 1 everywhere but db_out, whose scale sum |dy| is exact: the scales are sums of ABSOLUTE values carried through up to seven stages,
each a reduction over 24 .. 4160 terms whose rounding errors in fact add like a random walk; the worst ratios sit on the `const`, `sharp`,
`k_up` and ramp families, where they do not)

and K = ceil(4 x that), the project's margin (groupnorm_ref.py: the device's expf and division are a few ulp where the host's are at most 1,
FMA contraction moves single roundings, the order of the sum inside a matrix instruction is not ours to specify):

    K = {t_y: 1, t_dx: 1, t_dw: 1, t_dgamma: 1, t_dbias: 1,
         l_y_short: 1, l_y_long: 1, l_dx_short: 1, l_dx_long: 1, l_dw_short: 1, l_dw_long: 1, l_dgamma: 1, l_db_out: 6}
"""
import functools
import math

import torch

EPS = float(torch.tensor(1e-5, dtype=torch.float32))
U = 2.0 ** -24
FL = 2.0 ** -40
HEADS, DH, HD = 4, 32, 128
SCALE = DH ** -0.5
LONG = 1024
f64, f32 = torch.float64, torch.float32

K = {'t_y': 1, 't_dx': 1, 't_dw': 1, 't_dgamma': 1, 't_dbias': 1,
     'l_y_short': 1, 'l_y_long': 1, 'l_dx_short': 1, 'l_dx_long': 1, 'l_dw_short': 1, 'l_dw_long': 1, 'l_dgamma': 1, 'l_db_out': 6}
_T_KIND = {'y': 't_y', 'branch': 't_y', 'dx': 't_dx', 'dx_branch': 't_dx', 'dwq': 't_dw', 'dwo': 't_dw', 'dgamma': 't_dgamma', 'dbias': 't_dbias',
           'demb': 't_dbias'}
_L_KIND = {'y': 'l_y', 'branch': 'l_y', 'dx': 'l_dx', 'dx_branch': 'l_dx', 'dwq': 'l_dw', 'dwo': 'l_dw', 'dgamma': 'l_dgamma', 'db_out': 'l_db_out'}


def kind_t(name):
    return _T_KIND[name]


def kind_l(name, n_tok):
    k = _L_KIND[name]
    return k if k in ('l_dgamma', 'l_db_out') else k + ('_long' if n_tok >= LONG else '_short')


# ------------------------------------------------------------------------------------------------------------------ the case matrices
# Temporal: (C, B, F, H, W) -> the regime the case exists for, as the answers of ops.tattn_fused_plan (256 CUs: forward and wide grids
# min(512, nseq), 48-frame and backward grids min(256, nseq)); an entry lists only the keys the case exists for.
T_SHAPES = {'min': (1, 8, 8), 'one_pass': (3, 7, 11), 'carry': (9, 7, 11), 'hw_gt_grid': (1, 24, 23), 'grid_exact': (2, 16, 16), 'hw1': (300, 1, 1),
            'reduce_tail': (1, 3, 29)}
T_REGIME = {
    'min': dict(nseq=64, grid_fwd=64, passes_fwd=1, passes_bwd=1),                                  # the minimum ops.tattn_fused_takes admits
    'one_pass': dict(nseq=231, passes_fwd=1, passes_bwd=1, gstep_b_fwd=3, gstep_p_fwd=0),           # samples change inside the grid
    'carry': dict(nseq=693, passes_fwd=2, gstep_b_fwd=6, gstep_p_fwd=50, passes_bwd=3, gstep_b_bwd=3, gstep_p_bwd=25),
    'hw_gt_grid': dict(nseq=552, passes_fwd=2, gstep_b_fwd=0, passes_bwd=3, gstep_b_bwd=0),         # HW > grid
    'grid_exact': dict(nseq=512, grid_fwd=512, passes_fwd=1, passes_bwd=2, gstep_p_bwd=0),          # nseq == grid; two FULL passes backward
    'hw1': dict(nseq=300, gstep_p_fwd=0, gstep_b_fwd=300, passes_bwd=2, gstep_b_bwd=256, gstep_p_bwd=0),      # every step changes the sample
    # tattn_fused_reduce_kernel sums grid_bwd partials in eight chains, unrolled by 32 with a tail by 8: 64 and 256 partials have no tail,
    # 231 a tail of one, 87 two unrolled steps and a tail of three (two in the last chain)
    'reduce_tail': dict(nseq=87, grid_bwd=87, passes_bwd=1),
}
# 48 frames and the wide kernels: the backward entries do not apply; 48 frames runs the backward's grid (one block per CU)
T_REGIME_48 = {'min': dict(nseq=64, passes_fwd=1), 'carry': dict(nseq=693, passes_fwd=3, gstep_b_fwd=3, gstep_p_fwd=25),
               'hw_gt_grid': dict(nseq=552, passes_fwd=3, gstep_b_fwd=0)}


def t_case(c, f, name):
    return (c, T_SHAPES[name][0], f) + T_SHAPES[name][1:]


def t_regime(case):
    c, b, f, h, w = case
    name = next(k for k, v in T_SHAPES.items() if v == (b, h, w))
    if f == 48:
        return T_REGIME_48[name]
    return {k: v for k, v in T_REGIME[name].items() if c == 64 or not k.endswith('_bwd')}


# (case, input family, gradient family or None = forward only, rotary and bias?)
T_MATRIX = [(t_case(64, 24, n), 'gauss', 'gauss', True) for n in T_SHAPES]
T_MATRIX += [(t_case(64, 24, 'min'), fam, 'gauss', True) for fam in ('offset', 'const', 'sharp')]
T_MATRIX += [(t_case(64, 24, 'carry'), 'const', 'gauss', True), (t_case(64, 24, 'min'), 'gauss', 'gauss', False)]
# the running scales interact with the walk: the anchor (one sequence per block: tf_fit fires once), the three-pass case and HW = 1
T_MATRIX += [(t_case(64, 24, n), 'gauss', g, True) for n in ('min', 'carry') for g in ('ramp_up', 'ramp_down', 'wide_ramp', 'holes', 'zero')]
T_MATRIX += [(t_case(64, 24, 'hw1'), 'gauss', g, True) for g in ('ramp_up', 'holes')]
T_MATRIX += [(t_case(64, 48, n), 'gauss', None, True) for n in ('min', 'carry', 'hw_gt_grid')]
T_MATRIX += [(t_case(64, 48, 'min'), fam, None, True) for fam in ('offset', 'const', 'sharp')] + [(t_case(64, 48, 'min'), 'gauss', None, False)]
for _c in (128, 256):
    T_MATRIX += [(t_case(_c, 24, n), 'gauss', None, True) for n in ('min', 'carry', 'grid_exact')]
    T_MATRIX += [(t_case(_c, 24, 'min'), fam, None, True) for fam in ('offset', 'const', 'sharp')] + [(t_case(_c, 24, 'min'), 'gauss', None, False)]

# Linear: (C, B, F, H, W) -> regime as the answers of ops.lattn_fused_plan; `empty` = trailing chunks of the first cut without a tile,
# `last_tokens` = tokens of the last tile, `items_per_block` = ceil(units chunks2 / grid2)
L_SHAPES = {'min': (1, 2, 4, 8), 'one_token': (1, 2, 3, 11), 'one_chunk': (2, 3, 7, 11), 'empty': (1, 5, 20, 20), 'cap': (1, 2, 64, 64),
            'cap_empty': (1, 2, 64, 65), 'units': (32, 24, 10, 16), 'items': (4, 24, 20, 20)}
L_REGIME = {
    'min': dict(ntiles=1, chunks=1, tiles_per_chunk=1, last_tokens=32),
    'one_token': dict(ntiles=2, chunks=1, last_tokens=1),
    'one_chunk': dict(ntiles=3, chunks=1, tiles_per_chunk=3, chunks2=3),
    'empty': dict(ntiles=13, chunks=6, tiles_per_chunk=3, empty=1, last_tokens=16, chunks2=13),
    'cap': dict(ntiles=128, chunks=64, tiles_per_chunk=2, empty=0, chunks2=16),
    'cap_empty': dict(ntiles=130, chunks=64, tiles_per_chunk=3, empty=20),
    'units': dict(ntiles=5, chunks=1, tiles_per_chunk=5, chunks2=1, grid2=256, items_per_block=3),
    'items': dict(ntiles=13, chunks=6, chunks2=13, grid2=256, items_per_block=5),        # 96 units x 13 chunks on 256 blocks
}


def l_case(c, name):
    return (c,) + L_SHAPES[name]


def l_regime(case):
    name = next(k for k, v in L_SHAPES.items() if v == tuple(case[1:]))
    return {k: v for k, v in L_REGIME[name].items() if case[0] == 64 or k not in ('chunks2', 'grid2', 'items_per_block')}


def l_plan_view(plan, n_tok):
    """The derived entries of a regime from ops.lattn_fused_plan's answer and the shape."""
    out = dict(plan)
    live = -(-plan['ntiles'] // plan['tiles_per_chunk'])
    out['empty'] = plan['chunks'] - live
    out['last_tokens'] = n_tok - 32 * (plan['ntiles'] - 1)
    return out


L_MATRIX = [(l_case(64, n), 'gauss', 'gauss') for n in L_SHAPES]
L_MATRIX += [(l_case(64, 'min'), fam, 'gauss') for fam in ('offset', 'const', 'sharp')]
# the online rescale and the merge meet the order of max_n k across tiles and chunks: every chunked shape; one-hot softmaxes over the tokens
L_MATRIX += [(l_case(64, n), fam, 'gauss') for n in ('one_token', 'empty', 'cap_empty') for fam in ('k_up', 'k_down')]
L_MATRIX += [(l_case(64, 'empty'), fam, 'gauss') for fam in ('const', 'sharp')]
# the running scales of the second pass: one item per block (min), several tiles per item (cap), several items per block (units)
L_MATRIX += [(l_case(64, n), 'gauss', g) for n in ('min', 'empty') for g in ('ramp_up', 'ramp_down', 'wide_ramp', 'holes', 'zero')]
L_MATRIX += [(l_case(64, n), 'gauss', g) for n in ('cap', 'units') for g in ('ramp_up', 'ramp_down')]
for _c in (128, 256):
    L_MATRIX += [(l_case(_c, n), 'gauss', None) for n in ('min', 'one_token', 'empty', 'cap')]
    L_MATRIX += [(l_case(_c, 'min'), fam, None) for fam in ('offset', 'const', 'sharp')] + [(l_case(_c, 'empty'), 'k_up', None)]


def case_id(entry):
    case = entry[0]
    return 'c%d-%dx%dx%dx%d-' % case + '-'.join(str(e) for e in entry[1:])


# ------------------------------------------------------------------------------------------------------------------ inputs
def _gen(case, salt):
    return torch.Generator().manual_seed(salt + sum(p * v for p, v in zip((7, 1009, 31, 211, 13), case)))


def _x_family(x, family, rows_of):
    """x [B, F, H, W, C] of a family. rows_of(x) yields views whose rows the `const` family makes constant."""
    if family == 'offset':
        return (x - 0.2) / 3.0 + 20.0                                         # rows with mean 20, std 0.5
    if family == 'const':
        for v in rows_of(x):
            v[...] = v[..., :1].clone()
    return x


def _dy_family(dy, family, order, n_order):
    """dy of a gradient family. order: integer tensor broadcastable to dy, the position (0 .. n_order - 1) at which a block meets the element."""
    if family == 'gauss':
        return dy
    if family == 'zero':
        return torch.zeros_like(dy)
    if family == 'holes':
        keep = ((order // 3) % 3 != 0)                                         # stretches of three, the first stretch included
        return dy * keep
    span = {'ramp_up': 10.0, 'ramp_down': -10.0, 'wide_ramp': 30.0}[family]
    return dy * torch.exp2(span * order.double() / n_order)


@functools.lru_cache(maxsize=6)
def t_inputs(case, family='gauss', grad='gauss', rot_bias=True):
    """fp32 CPU tensors of a temporal case (shared: read-only): x, gamma, wq [384, C], wo [C, 128], freqs [16] | None, emb [32, 4] | None, dy."""
    c, b, f, h, w = case
    gen = _gen(case, 17)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=f64)
    u = lambda *s: torch.rand(*s, generator=gen, dtype=f64) * 2 - 1
    x = r(b, f, h, w, c) * 1.5 + 0.2
    nseq = b * h * w

    def rows_of(x_):                                                           # a few sequences whose rows are each constant
        for s in sorted({0, nseq // 2, nseq - 1}):
            bi, pix = divmod(s, h * w)
            yield x_[bi, :, pix // w, pix % w, :]
    x = _x_family(x, family, rows_of)
    out = dict(x=x, gamma=1 + 0.3 * r(c), wq=u(3 * HD, c) / math.sqrt(c) * (16.0 if family == 'sharp' else 2.0), wo=u(c, HD) / math.sqrt(HD))
    out['freqs'] = 1.0 / (10000 ** (torch.arange(0, DH, 2).float() / DH)) if rot_bias else None
    out['emb'] = r(32, HEADS) if rot_bias else None
    if grad is not None:
        seq = (torch.arange(b)[:, None, None] * (h * w) + torch.arange(h)[None, :, None] * w + torch.arange(w)[None, None, :])[:, None, :, :, None]
        out['dy'] = _dy_family(r(b, f, h, w, c), grad, seq, nseq)
    return {k: (v if v is None else v.float()) for k, v in out.items()}


@functools.lru_cache(maxsize=6)
def l_inputs(case, family='gauss', grad='gauss'):
    """fp32 CPU tensors of a linear-attention case: x, gamma, wq [384, C], wo [C, 128], bo [C], dy."""
    c, b, f, h, w = case
    gen = _gen(case, 29)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=f64)
    u = lambda *s: torch.rand(*s, generator=gen, dtype=f64) * 2 - 1
    x = r(b, f, h, w, c) * 1.5 + 0.2
    n = h * w

    def rows_of(x_):                                                           # one whole frame constant, single constant rows elsewhere
        yield x_[0, f - 1]
        yield x_[0, 0, 0, :1]
        yield x_[b - 1, 0, h - 1, w - 1:]
    x = _x_family(x, family, rows_of)
    wq = u(3 * HD, c) / math.sqrt(c) * (24.0 if family == 'sharp' else 3.0)
    if family in ('k_up', 'k_down'):                                           # max_n k ascends / descends across the token tiles (LayerNorm removes a
        tok = torch.arange(n, dtype=f64).reshape(1, 1, h, w, 1) / n            # row's size, not its direction): a fixed direction u grows in along the tokens,
        x = 0.3 * x + 3.0 * (tok if family == 'k_up' else 1 - tok) * r(c)      # so every k[d] = W_k[d] xn drifts with the sign of W_k[d] . u -- both ways in one input
    out = dict(x=x, gamma=1 + 0.3 * r(c), wq=wq, wo=u(c, HD) / math.sqrt(HD), bo=u(c) / math.sqrt(HD))
    if grad is not None:
        order = torch.arange(n).reshape(1, 1, h, w, 1)
        out['dy'] = _dy_family(r(b, f, h, w, c), grad, order, n)
    return {k: (v if v is None else v.float()) for k, v in out.items()}


def rot_tables(freqs, n, dtype=f64):
    """cos / sin [n, 32] of the interleaved-pair rotary embedding (ops.rotary_tables)."""
    ang = (torch.arange(n, dtype=freqs.dtype)[:, None] * freqs[None, :]).repeat_interleave(2, dim=-1)
    return ang.cos().to(dtype), ang.sin().to(dtype)


def bias_table(emb, n):
    """[heads, n, n] relative-position bias and its bucket table [n, n] (the integer table of conv3d.py:86-112)."""
    from oracle.unet_ref import relative_position_bucket
    pos = torch.arange(n)
    bucket = relative_position_bucket(pos[None, :] - pos[:, None])
    return emb[bucket].permute(2, 0, 1), bucket


# ------------------------------------------------------------------------------------------------------------------ shared stages (fp64)
def _ln(x, gamma):
    """LayerNorm over the last axis (biased variance, gain only): xh, rstd, mean, xs_h = scale of xh."""
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + EPS)
    return (x - mean) * rstd, rstd, mean, (x.abs() + mean.abs()) * rstd


def _heads(t):
    """[..., n, 128] -> [..., 4, n, 32]"""
    return t.reshape(*t.shape[:-1], HEADS, DH).transpose(-2, -3)


def _unheads(t):
    return t.transpose(-2, -3).reshape(*t.shape[:-3], t.shape[-2], HD)


def _rot(t, cos, sin, inverse=False):
    """rotation of the pairs (2i, 2i + 1) of the last axis by the angles of the token axis (-2); inverse: its transpose (the gradient)."""
    x, y = t[..., 0::2], t[..., 1::2]
    c, s = cos[:, 0::2], sin[:, 0::2]
    if inverse:
        s = -s
    return torch.stack((x * c - y * s, y * c + x * s), dim=-1).reshape(t.shape)


def _rot_abs(t, cos, sin):
    x, y = t[..., 0::2], t[..., 1::2]
    c, s = cos[:, 0::2].abs(), sin[:, 0::2].abs()
    return torch.stack((x * c + y * s, y * c + x * s), dim=-1).reshape(t.shape)


def _ln_backward(dxn, s_dxn, fl_dxn, xh, xs_h, rstd, gam, dy):
    """LayerNorm backward + residual gradient: (dx, dxl, dgamma-terms) and their scales; sums over rows are left to the caller."""
    c = xh.shape[-1]
    dn, s_dn = dxn * gam, s_dxn * gam.abs()
    m1, m2 = dn.mean(-1, keepdim=True), (dn * xh).mean(-1, keepdim=True)
    s_m1 = s_dn.mean(-1, keepdim=True)
    s_m2 = (s_dn * xh.abs() + dn.abs() * xs_h).mean(-1, keepdim=True)
    dxl = rstd * (dn - m1 - xh * m2)
    s_dxl = rstd * (s_dn + s_m1 + xh.abs() * s_m2 + xs_h * m2.abs()) + dxl.abs()
    fl_dn = fl_dxn * gam.abs()
    fl = rstd * (fl_dn + fl_dn.mean(-1, keepdim=True) + xh.abs() * (fl_dn * xh.abs()).mean(-1, keepdim=True))
    dx = dxl + dy
    return dict(dx=dx, dx_branch=dxl, dg=dxn * xh), dict(dx=s_dxl + dx.abs(), dx_branch=s_dxl, dg=s_dxn * xh.abs() + dxn.abs() * xs_h), \
        dict(dx=fl, dx_branch=fl, dg=fl_dxn * xh.abs())


def _amax(t):
    return float(t.abs().max())


def _prod_flush(a, b, contract):
    """flush of a plane product: 2^-40 (amax(a) sum |b| + amax(b) sum |a|), `contract(a_, b_)` doing the contraction on |.| tensors."""
    return FL * (contract(torch.full_like(a, _amax(a)), b.abs()) + contract(a.abs(), torch.full_like(b, _amax(b))))


# ------------------------------------------------------------------------------------------------------------------ temporal reference
def to_seq(t):
    """[B, F, H, W, C] -> [B H W, F, C]"""
    b, f, h, w, c = t.shape
    return t.permute(0, 2, 3, 1, 4).reshape(b * h * w, f, c)


def from_seq(t, shape):
    b, f, h, w, c = shape
    return t.reshape(b, h, w, f, c).permute(0, 3, 1, 2, 4)


def reference_t(x, gamma, wq, wo, freqs=None, emb=None, dy=None):
    """fp64 outputs, scales and flush terms of the temporal block: ({name: tensor}, {name: scale}, {name: flush}, info). Forward: y, branch
    (= y - x). With dy: dx, dx_branch (= dx - dy), dgamma, dwq, dwo and, with emb, dbias [4, F, F] and demb [32, 4]. Activations come back in
    the shape of x."""
    shape = x.shape
    f = shape[1]
    xq, gam, Wq, Wo = to_seq(x.double()), gamma.double().reshape(-1), wq.double(), wo.double()
    cos, sin = rot_tables(freqs.double(), f) if freqs is not None else (torch.ones(f, DH, dtype=f64), torch.zeros(f, DH, dtype=f64))
    bias, bucket = bias_table(emb.double(), f) if emb is not None else (torch.zeros(HEADS, f, f, dtype=f64), None)
    xh, rstd, mean, xs_h = _ln(xq, gam)
    xn, xs = xh * gam, xs_h * gam.abs()
    qkv, s_qkv = xn @ Wq.T, xs @ Wq.abs().T
    fl_qkv = _prod_flush(xn, Wq, lambda a_, b_: a_ @ b_.T)
    q, k, v = (_heads(t) for t in qkv.chunk(3, -1))
    s_q, s_k, s_v = (_heads(t) for t in s_qkv.chunk(3, -1))
    fl_q, fl_k, fl_v = (_heads(t) for t in fl_qkv.chunk(3, -1))
    q, s_q, fl_q = _rot(q * SCALE, cos, sin), _rot_abs(s_q * SCALE, cos, sin), _rot_abs(fl_q * SCALE, cos, sin)
    k, s_k, fl_k = _rot(k, cos, sin), _rot_abs(s_k, cos, sin), _rot_abs(fl_k, cos, sin)
    kt = k.transpose(-1, -2)
    lg = q @ kt + bias
    s_lg = s_q @ kt.abs() + q.abs() @ s_k.transpose(-1, -2) + bias.abs()
    fl_lg = fl_q @ kt.abs() + q.abs() @ fl_k.transpose(-1, -2)
    p = torch.softmax(lg, -1)
    s_p = p * (1 + s_lg + (p * s_lg).sum(-1, keepdim=True))
    fl_p = p * (fl_lg + (p * fl_lg).sum(-1, keepdim=True))
    o, s_o, fl_o = p @ v, s_p @ v.abs() + p @ s_v, fl_p @ v.abs() + p @ fl_v
    of, s_of, fl_of = _unheads(o), _unheads(s_o), _unheads(fl_o)
    br, s_br = of @ Wo.T, s_of @ Wo.abs().T
    fl_br = fl_of @ Wo.abs().T + _prod_flush(of, Wo, lambda a_, b_: a_ @ b_.T)
    y = br + xq
    back = lambda t: from_seq(t, shape)
    out = {'y': back(y), 'branch': back(br)}
    scale = {'y': back(s_br + y.abs()), 'branch': back(s_br)}
    flush = {'y': back(fl_br), 'branch': back(fl_br)}
    info = {'amax_y': _amax(y)}
    if dy is None:
        return out, scale, flush, info
    g = to_seq(dy.double())
    do, s_do = _heads(g @ Wo), _heads(g.abs() @ Wo.abs())
    fl_do = _heads(_prod_flush(g, Wo, lambda a_, b_: a_ @ b_))
    gf, sf = g.reshape(-1, g.shape[-1]), s_of.reshape(-1, HD)
    out['dwo'], scale['dwo'] = gf.T @ of.reshape(-1, HD), gf.abs().T @ sf
    flush['dwo'] = gf.abs().T @ fl_of.reshape(-1, HD) + _prod_flush(gf, of.reshape(-1, HD), lambda a_, b_: a_.T @ b_)
    vt = v.transpose(-1, -2)
    dp, s_dp, fl_dp = do @ vt, s_do @ vt.abs() + do.abs() @ s_v.transpose(-1, -2), fl_do @ vt.abs() + do.abs() @ fl_v.transpose(-1, -2)
    pt = p.transpose(-1, -2)
    dv, s_dv, fl_dv = pt @ do, s_p.transpose(-1, -2) @ do.abs() + pt @ s_do, fl_p.transpose(-1, -2) @ do.abs() + pt @ fl_do
    delta = (p * dp).sum(-1, keepdim=True)
    s_delta = (s_p * dp.abs() + p * s_dp).sum(-1, keepdim=True)
    fl_delta = (fl_p * dp.abs() + p * fl_dp).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    s_ds = s_p * (dp.abs() + delta.abs()) + p * (s_dp + s_delta)
    fl_ds = fl_p * (dp.abs() + delta.abs()) + p * (fl_dp + fl_delta)
    if emb is not None:
        out['dbias'], scale['dbias'], flush['dbias'] = ds.sum(0), s_ds.sum(0), fl_ds.sum(0)
        scat = lambda t: torch.zeros(32, HEADS, dtype=f64).index_add_(0, bucket.reshape(-1), t.permute(1, 2, 0).reshape(-1, HEADS))
        out['demb'], scale['demb'], flush['demb'] = scat(out['dbias']), scat(scale['dbias']), scat(flush['dbias'])
    dst = ds.transpose(-1, -2)
    dq, s_dq, fl_dq = ds @ k, s_ds @ k.abs() + ds.abs() @ s_k, fl_ds @ k.abs() + ds.abs() @ fl_k
    dk, s_dk, fl_dk = dst @ q, s_ds.transpose(-1, -2) @ q.abs() + dst.abs() @ s_q, fl_ds.transpose(-1, -2) @ q.abs() + dst.abs() @ fl_q
    dq, s_dq, fl_dq = _rot(dq, cos, sin, True) * SCALE, _rot_abs(s_dq, cos, sin) * SCALE, _rot_abs(fl_dq, cos, sin) * SCALE
    dk, s_dk, fl_dk = _rot(dk, cos, sin, True), _rot_abs(s_dk, cos, sin), _rot_abs(fl_dk, cos, sin)
    tail = _qkv_tail([dq, dk, dv], [s_dq, s_dk, s_dv], [fl_dq, fl_dk, fl_dv], xn, xs, xh, xs_h, rstd, gam, Wq, g)
    for part, dst_ in zip(tail, (out, scale, flush)):
        for name, t in part.items():
            dst_[name] = back(t) if name in ('dx', 'dx_branch') else t
    info['amax_dx'] = _amax(out['dx'])
    return out, scale, flush, info


def _qkv_tail(d, s_d, fl_d, xn, xs, xh, xs_h, rstd, gam, Wq, g):
    """From the gradients of (q, k, v) per head [..., 4, n, 32] to dwq, dgamma, dx, dx_branch: three dicts (values, scales, flushes)."""
    dqkv = torch.cat([_unheads(t) for t in d], -1)
    s_dqkv = torch.cat([_unheads(t) for t in s_d], -1)
    fl_in = torch.cat([_unheads(t) for t in fl_d], -1)
    # the planes of dq / dk / dv carry one scale per tensor (and wave): amax per tensor, the global maximum (module docstring)
    am = torch.cat([torch.full((HD,), _amax(t), dtype=f64) for t in d])
    df, sf, xf, xsf = dqkv.reshape(-1, 3 * HD), s_dqkv.reshape(-1, 3 * HD), xn.reshape(-1, xn.shape[-1]), xs.reshape(-1, xn.shape[-1])
    ff = fl_in.reshape(-1, 3 * HD)
    out = {'dwq': df.T @ xf}
    scale = {'dwq': sf.T @ xf.abs() + df.abs().T @ xsf}
    flush = {'dwq': ff.T @ xf.abs() + FL * (am[:, None] * xf.abs().sum(0)[None, :] + _amax(xn) * df.abs().sum(0)[:, None])}
    dxn, s_dxn = dqkv @ Wq, s_dqkv @ Wq.abs()
    fl_dxn = fl_in @ Wq.abs() + FL * ((am[:, None] * Wq.abs()).sum(0) + _amax(Wq) * dqkv.abs().sum(-1, keepdim=True))
    o_, s_, f_ = _ln_backward(dxn, s_dxn, fl_dxn, xh, xs_h, rstd, gam, g)
    red = lambda t: t.reshape(-1, t.shape[-1]).sum(0)
    out.update(dx=o_['dx'], dx_branch=o_['dx_branch'], dgamma=red(o_['dg']))
    scale.update(dx=s_['dx'], dx_branch=s_['dx_branch'], dgamma=red(s_['dg']))
    flush.update(dx=f_['dx'], dx_branch=f_['dx_branch'], dgamma=red(f_['dg']))
    return out, scale, flush


# ------------------------------------------------------------------------------------------------------------------ linear reference
def to_units(t):
    b, f, h, w, c = t.shape
    return t.reshape(b * f, h * w, c)


def reference_l(x, gamma, wq, wo, bo=None, dy=None):
    """fp64 outputs, scales and flush terms of the linear-attention block, as reference_t: y, branch; with dy dx, dx_branch, dgamma, dwq, dwo,
    db_out."""
    shape = x.shape
    xq, gam, Wq, Wo = to_units(x.double()), gamma.double().reshape(-1), wq.double().reshape(3 * HD, -1), wo.double().reshape(-1, HD)
    b_ = bo.double() if bo is not None else torch.zeros(shape[-1], dtype=f64)
    xh, rstd, mean, xs_h = _ln(xq, gam)
    xn, xs = xh * gam, xs_h * gam.abs()
    qkv, s_qkv = xn @ Wq.T, xs @ Wq.abs().T
    fl_qkv = _prod_flush(xn, Wq, lambda a_, b_: a_ @ b_.T)
    q, k, v = (_heads(t) for t in qkv.chunk(3, -1))                                # [U, 4, n, 32]
    s_q, s_k, s_v = (_heads(t) for t in s_qkv.chunk(3, -1))
    fl_q, fl_k, fl_v = (_heads(t) for t in fl_qkv.chunk(3, -1))
    sm = torch.softmax(q, -1)
    qs = sm * SCALE
    s_qs = qs * (1 + s_q + (sm * s_q).sum(-1, keepdim=True))
    fl_qs = qs * (fl_q + (sm * fl_q).sum(-1, keepdim=True))
    ks = torch.softmax(k, -2)
    s_ks = ks * (1 + s_k + (ks * s_k).sum(-2, keepdim=True))
    fl_ks = ks * (fl_k + (ks * fl_k).sum(-2, keepdim=True))
    kst = ks.transpose(-1, -2)
    ctx, s_ctx, fl_ctx = kst @ v, s_ks.transpose(-1, -2) @ v.abs() + kst @ s_v, fl_ks.transpose(-1, -2) @ v.abs() + kst @ fl_v      # [U, 4, d, e]
    o, s_o, fl_o = qs @ ctx, s_qs @ ctx.abs() + qs @ s_ctx, fl_qs @ ctx.abs() + qs @ fl_ctx
    of, s_of, fl_of = _unheads(o), _unheads(s_o), _unheads(fl_o)
    br, s_br = of @ Wo.T + b_, s_of @ Wo.abs().T + b_.abs()
    fl_br = fl_of @ Wo.abs().T + _prod_flush(of, Wo, lambda a_, b2: a_ @ b2.T)
    y = br + xq
    back = lambda t: t.reshape(shape)
    out = {'y': back(y), 'branch': back(br)}
    scale = {'y': back(s_br + y.abs()), 'branch': back(s_br)}
    flush = {'y': back(fl_br), 'branch': back(fl_br)}
    info = {'amax_y': _amax(y)}
    if dy is None:
        return out, scale, flush, info
    g = to_units(dy.double())
    do, s_do = _heads(g @ Wo), _heads(g.abs() @ Wo.abs())
    fl_do = _heads(_prod_flush(g, Wo, lambda a_, b2: a_ @ b2))
    gf = g.reshape(-1, g.shape[-1])
    out['dwo'], scale['dwo'] = gf.T @ of.reshape(-1, HD), gf.abs().T @ s_of.reshape(-1, HD)
    flush['dwo'] = gf.abs().T @ fl_of.reshape(-1, HD) + _prod_flush(gf, of.reshape(-1, HD), lambda a_, b2: a_.T @ b2)
    out['db_out'], scale['db_out'], flush['db_out'] = gf.sum(0), gf.abs().sum(0), torch.zeros_like(b_)
    qst = qs.transpose(-1, -2)
    dctx, s_dctx, fl_dctx = qst @ do, s_qs.transpose(-1, -2) @ do.abs() + qst @ s_do, fl_qs.transpose(-1, -2) @ do.abs() + qst @ fl_do
    ctxt = ctx.transpose(-1, -2)
    dqs = do @ ctxt
    s_dqs, fl_dqs = s_do @ ctxt.abs() + do.abs() @ s_ctx.transpose(-1, -2), fl_do @ ctxt.abs() + do.abs() @ fl_ctx.transpose(-1, -2)
    inner = (qs * dqs).sum(-1, keepdim=True) / SCALE
    s_inner = (s_qs * dqs.abs() + qs * s_dqs).sum(-1, keepdim=True) / SCALE
    fl_inner = (fl_qs * dqs.abs() + qs * fl_dqs).sum(-1, keepdim=True) / SCALE
    dq = qs * (dqs - inner)
    s_dq = s_qs * (dqs.abs() + inner.abs()) + qs * (s_dqs + s_inner)
    fl_dq = fl_qs * (dqs.abs() + inner.abs()) + qs * (fl_dqs + fl_inner)
    dctxt = dctx.transpose(-1, -2)
    dks = v @ dctxt                                                               # [U, 4, n, d]
    s_dks, fl_dks = s_v @ dctxt.abs() + v.abs() @ s_dctx.transpose(-1, -2), fl_v @ dctxt.abs() + v.abs() @ fl_dctx.transpose(-1, -2)
    T = (dctx * ctx).sum(-1)[..., None, :]                                        # [U, 4, 1, d]
    s_T = (s_dctx * ctx.abs() + dctx.abs() * s_ctx).sum(-1)[..., None, :]
    fl_T = (fl_dctx * ctx.abs() + dctx.abs() * fl_ctx).sum(-1)[..., None, :]
    dk = ks * (dks - T)
    s_dk = s_ks * (dks.abs() + T.abs()) + ks * (s_dks + s_T)
    fl_dk = fl_ks * (dks.abs() + T.abs()) + ks * (fl_dks + fl_T)
    dv, s_dv, fl_dv = ks @ dctx, s_ks @ dctx.abs() + ks @ s_dctx, fl_ks @ dctx.abs() + ks @ fl_dctx
    tail = _qkv_tail([dq, dk, dv], [s_dq, s_dk, s_dv], [fl_dq, fl_dk, fl_dv], xn, xs, xh, xs_h, rstd, gam, Wq, g)
    for part, dst_ in zip(tail, (out, scale, flush)):
        for name, t in part.items():
            dst_[name] = back(t) if name in ('dx', 'dx_branch') else t
    info['amax_dx'] = _amax(out['dx'])
    return out, scale, flush, info


@functools.lru_cache(maxsize=4)
def reference_of_t(entry):
    case, family, grad, rot_bias = entry
    t = t_inputs(case, family, grad, rot_bias)
    return reference_t(t['x'], t['gamma'], t['wq'], t['wo'], t['freqs'], t['emb'], t.get('dy'))


@functools.lru_cache(maxsize=4)
def reference_of_l(entry):
    case, family, grad = entry
    t = l_inputs(case, family, grad)
    return reference_l(t['x'], t['gamma'], t['wq'], t['wo'], t['bo'], t.get('dy'))


# ------------------------------------------------------------------------------------------------------------------ the kernels' arithmetic, fp32
def scale_from_amax(amax):
    """csrc/common.h: the power of two that brings amax into [2^14, 2^15); 1 for 0 and non-finite values."""
    amax = float(amax)
    if not (amax > 0.0) or not math.isfinite(amax):
        return 1.0
    return 2.0 ** (14 - math.frexp(amax)[1] + 1)


def _scale_from_amax_t(am):
    """scale_from_amax element-wise on an fp32 tensor"""
    e = torch.floor(torch.log2(am.double().clamp_min(1e-300)))
    return torch.where(am > 0, torch.exp2(14 - e), torch.ones_like(e)).float()


def tf_scale(bound):
    return min(max(scale_from_amax(bound), 2.0 ** -100), 2.0 ** 100)


def planes(t, s):
    """(hi, lo) fp16 planes of fp32 t at the power-of-two scale s (a float or a broadcastable tensor), returned as fp32 values."""
    ts = t * s
    hi = ts.half().float()
    return hi, (ts - hi).half().float()


def mm3(a, b, contract):
    """the three plane products hi lo + lo hi + hi hi in fp32, accumulated in the kernels' order; a, b = (hi, lo) pairs"""
    return (contract(a[0], b[1]) + contract(a[1], b[0])) + contract(a[0], b[0])


def _ln32(x, gam, c):
    mean = x.sum(-1, keepdim=True) * (1.0 / c)
    xc = x - mean
    rstd = 1.0 / torch.sqrt((xc * xc).sum(-1, keepdim=True) * (1.0 / c) + EPS)
    return xc * rstd, rstd, xc * rstd * gam


def _softmax32(t, dim, mul=1.0):
    e = torch.exp(t - t.amax(dim, keepdim=True))
    return e * (mul / e.sum(dim, keepdim=True))


def _ln_backward32(parts, xh, rstd, gam, g):
    """parts: per-head partial dxn tiles [..., 4, n, C]; heads summed (a + b) + (c + d), LayerNorm backward, residual gradient."""
    c = xh.shape[-1]
    dn = (parts[..., 0, :, :] + parts[..., 1, :, :]) + (parts[..., 2, :, :] + parts[..., 3, :, :])
    dg = dn * xh
    dn = dn * gam
    m1 = dn.sum(-1, keepdim=True) * (1.0 / c)
    m2 = (dn * xh).sum(-1, keepdim=True) * (1.0 / c)
    return rstd * (dn - m1 - xh * m2) + g, dg


def _qkv_tail32(d, xh, rstd, gam, ps, xp, Wp, sw, g, scales=None):
    """dq / dk / dv [..., 4, n, 32] fp32 -> dwq, dx, dgamma as the backward kernels form them: planes per tensor and head at the scale of
    the tensor's largest tile (the running scale's final value), weight gradient and dxn on the three plane products."""
    c = xh.shape[-1]
    dwq = torch.empty(3, HEADS, DH, c, dtype=f32)
    parts = torch.zeros(*d[0].shape[:-1], c, dtype=f32)
    wp = [w_.reshape(3, HEADS, DH, c) for w_ in Wp]
    xf = [t.reshape(-1, c) for t in xp]
    for ti, t in enumerate(d):
        for h in range(HEADS):
            th = t[..., h, :, :]
            sc = tf_scale(_amax(th)) if scales is None else scales[ti][h]
            dp_ = planes(th, sc)
            df = [p_.reshape(-1, DH) for p_ in dp_]
            dwq[ti, h] = mm3(df, xf, lambda a_, b_: a_.T @ b_) * (1.0 / (sc * ps))
            parts[..., h, :, :] = mm3(dp_, (wp[0][ti, h], wp[1][ti, h]), lambda a_, b_: a_ @ b_) * (1.0 / (sc * sw)) + parts[..., h, :, :]
    dx, dg = _ln_backward32(parts, xh, rstd, gam, g)
    return dwq.reshape(3 * HD, c), dx, dg.reshape(-1, c).sum(0)


def transcription_t(x, gamma, wq, wo, freqs=None, emb=None, dy=None):
    """The temporal kernels' arithmetic in fp32 torch (module docstring); {name: fp32 tensor} like reference_t."""
    shape = x.shape
    f, c = shape[1], shape[-1]
    xq, gam, Wq, Wo = to_seq(x.float()), gamma.float().reshape(-1), wq.float(), wo.float()
    cos, sin = rot_tables(freqs.float(), f, f32) if freqs is not None else (torch.ones(f, DH), torch.zeros(f, DH))
    bias, bucket = bias_table(emb.float(), f) if emb is not None else (torch.zeros(HEADS, f, f), None)
    xh, rstd, xn = _ln32(xq, gam, c)
    ps, sw, swo = scale_from_amax(math.sqrt(c) * _amax(gam)), scale_from_amax(_amax(Wq)), scale_from_amax(_amax(Wo))
    xp, Wp, Wop = planes(xn, ps), planes(Wq, sw), planes(Wo, swo)
    qkv = mm3(xp, Wp, lambda a_, b_: a_ @ b_.T) * (1.0 / (ps * sw))
    q, k, v = (_heads(t) for t in qkv.chunk(3, -1))
    q, k = _rot(q * SCALE, cos, sin), _rot(k, cos, sin)
    p = _softmax32(q @ k.transpose(-1, -2) + bias, -1)
    o = p @ v
    # to_out per head at the scale of max|v| of the (sequence, head) -- of the sequence at 128 / 256 channels --, partials summed (a + b) + (c + d)
    amv = v.abs().amax((-1, -2), keepdim=True)
    if c != 64:
        amv = amv.amax(1, keepdim=True).expand_as(amv)
    so = _scale_from_amax_t(amv)
    op = planes(o, so)
    wo_h = [w_.reshape(c, HEADS, DH).permute(1, 2, 0) for w_ in Wop]                 # [4, 32, C]
    part = mm3(op, wo_h, lambda a_, b_: a_ @ b_) * (1.0 / (so * swo))               # [S, 4, F, C]
    br = (part[:, 0] + part[:, 1]) + (part[:, 2] + part[:, 3])
    y = br + xq
    back = lambda t: from_seq(t, shape)
    out = {'y': back(y), 'branch': back(y - xq)}
    if dy is None:
        return out
    g = to_seq(dy.float())
    sc_g, sc_o = tf_scale(_amax(g)), tf_scale(_amax(v))
    gp = planes(g, sc_g)
    do = _heads(mm3(gp, Wop, lambda a_, b_: a_ @ b_) * (1.0 / (sc_g * swo)))
    dp = do @ v.transpose(-1, -2)
    delta = (p * dp).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    if emb is not None:
        out['dbias'] = ds.sum(0)
        out['demb'] = torch.zeros(32, HEADS).index_add_(0, bucket.reshape(-1), out['dbias'].permute(1, 2, 0).reshape(-1, HEADS))
    dq, dk, dv = _rot(ds @ k, cos, sin, True) * SCALE, _rot(ds.transpose(-1, -2) @ q, cos, sin, True), p.transpose(-1, -2) @ do
    opb = [_unheads(t).reshape(-1, HD) for t in planes(o, sc_o)]
    out['dwo'] = mm3([t.reshape(-1, c) for t in gp], opb, lambda a_, b_: a_.T @ b_) * (1.0 / (sc_g * sc_o))
    out['dwq'], dx, out['dgamma'] = _qkv_tail32([dq, dk, dv], xh, rstd, gam, ps, xp, Wp, sw, g)
    out['dx'] = back(dx)
    out['dx_branch'] = back(dx - g)
    return out


def transcription_l(x, gamma, wq, wo, bo=None, dy=None, plan=None):
    """The linear-attention kernels' arithmetic in fp32 torch. plan = dict(chunks, tiles_per_chunk): the cut of a frame (ops.lattn_fused_plan); the
    context is accumulated tile by tile with the online softmax inside a chunk and merged over the chunks in chunk order."""
    shape = x.shape
    c = shape[-1]
    xq, gam, Wq, Wo = to_units(x.float()), gamma.float().reshape(-1), wq.float().reshape(3 * HD, -1), wo.float().reshape(-1, HD)
    b_ = bo.float() if bo is not None else torch.zeros(c)
    units, n = xq.shape[:2]
    xh, rstd, xn = _ln32(xq, gam, c)
    ps, sw, swo = scale_from_amax(math.sqrt(c) * _amax(gam)), scale_from_amax(_amax(Wq)), scale_from_amax(_amax(Wo))
    xp, Wp, Wop = planes(xn, ps), planes(Wq, sw), planes(Wo, swo)
    qkv = mm3(xp, Wp, lambda a_, b_: a_ @ b_.T) * (1.0 / (ps * sw))
    q, k, v = (_heads(t) for t in qkv.chunk(3, -1))                                # [U, 4, n, 32]
    chunks, tpc = plan['chunks'], plan['tiles_per_chunk']
    npad = chunks * tpc * 32
    pad = lambda t, val: torch.cat([t, torch.full((units, HEADS, npad - n, DH), val)], 2).reshape(units, HEADS, chunks, tpc, 32, DH)
    kc, vc = pad(k, -math.inf), pad(v, 0.0)
    m_run = torch.full((units, HEADS, chunks, DH), -math.inf)
    z_run = torch.zeros(units, HEADS, chunks, DH)
    craw = torch.zeros(units, HEADS, chunks, DH, DH)
    for t in range(tpc):
        kt, vt = kc[:, :, :, t], vc[:, :, :, t]                                    # [U, 4, chunks, 32 tokens, 32]
        m_new = torch.maximum(m_run, kt.amax(-2))
        fac = torch.where(torch.isinf(m_run), torch.zeros_like(m_run), torch.exp(m_run - m_new))
        fac = torch.where(m_new == m_run, torch.ones_like(fac), fac)
        z_run, craw, m_run = z_run * fac, craw * fac[..., None], m_new
        e = torch.where(torch.isinf(kt), torch.zeros_like(kt), torch.exp(kt - m_run[..., None, :]))
        z_run = z_run + e.sum(-2)
        craw = craw + e.transpose(-1, -2) @ vt
    M = m_run.amax(2)
    Z, ctx = torch.zeros(units, HEADS, DH), torch.zeros(units, HEADS, DH, DH)
    for ci in range(chunks):
        wgt = torch.where(torch.isinf(m_run[:, :, ci]), torch.zeros_like(M), torch.exp(m_run[:, :, ci] - M))
        Z, ctx = Z + z_run[:, :, ci] * wgt, ctx + craw[:, :, ci] * wgt[..., None]
    ctx = ctx / Z[..., None]
    qs = _softmax32(q, -1, SCALE)
    o = qs @ ctx
    amc = ctx.abs().amax((-1, -2), keepdim=True)
    if c != 64:
        amc = amc.amax(1, keepdim=True).expand_as(amc)
    so = _scale_from_amax_t(SCALE * amc)
    wo_h = [w_.reshape(c, HEADS, DH).permute(1, 2, 0) for w_ in Wop]
    part = mm3(planes(o, so), wo_h, lambda a_, b2: a_ @ b2) * (1.0 / (so * swo))
    br = ((part[:, 0] + part[:, 1]) + (part[:, 2] + part[:, 3])) + b_
    y = br + xq
    back = lambda t: t.reshape(shape)
    out = {'y': back(y), 'branch': back(y - xq)}
    if dy is None:
        return out
    g = to_units(dy.float())
    sc_g = tf_scale(_amax(g))
    gp = planes(g, sc_g)
    do = _heads(mm3(gp, Wop, lambda a_, b2: a_ @ b2) * (1.0 / (sc_g * swo)))
    # dctx per chunk of the first cut, chunks summed in chunk order
    padz = lambda t: torch.cat([t, torch.zeros(units, HEADS, npad - n, DH)], 2).reshape(units, HEADS, chunks, tpc * 32, DH)
    pc = padz(qs).transpose(-1, -2) @ padz(do)
    dctx = torch.zeros(units, HEADS, DH, DH)
    for ci in range(chunks):
        dctx = dctx + pc[:, :, ci]
    T = (dctx * ctx).sum(-1)[..., None, :]
    ks = torch.exp(k - M[..., None, :]) * (1.0 / Z)[..., None, :]
    dqs = do @ ctx.transpose(-1, -2)
    inner = (qs * dqs).sum(-1, keepdim=True) * (1.0 / SCALE)
    dq = qs * (dqs - inner)
    dk = ks * (v @ dctx.transpose(-1, -2) - T)
    dv = ks @ dctx
    sc_o = [tf_scale(SCALE * _amax(ctx[:, h])) for h in range(HEADS)]
    opl = [torch.stack([planes(o[:, h], sc_o[h])[i] / sc_o[h] for h in range(HEADS)], 1) for i in (0, 1)]      # planes per head, back in value units
    out['dwo'] = mm3([t.reshape(-1, c) for t in gp], [_unheads(t).reshape(-1, HD) for t in opl], lambda a_, b2: a_.T @ b2) * (1.0 / sc_g)
    out['db_out'] = g.reshape(-1, c).sum(0)
    out['dwq'], dx, out['dgamma'] = _qkv_tail32([dq, dk, dv], xh, rstd, gam, ps, xp, Wp, sw, g)
    out['dx'] = back(dx)
    out['dx_branch'] = back(dx - g)
    return out


def transcription(block, *args, **kwargs):
    """transcription_t ('temporal') or transcription_l ('linear')"""
    return {'temporal': transcription_t, 'linear': transcription_l}[block](*args, **kwargs)


# ------------------------------------------------------------------------------------------------------------------ the gate
def ratio(got, ref, scale, flush=None):
    """max of (|got - ref| - flush) / (2^-24 scale)"""
    err = (got.detach().double().cpu().reshape(ref.shape) - ref).abs()
    if flush is not None:
        err = (err - flush).clamp_min(0)
    if not torch.isfinite(err).all():
        return math.inf
    r = err / (U * scale).clamp_min(1e-300)
    return float(r.max())


def ratios(got, ref):
    """{name: ratio} of every output in `got` against ref = (out, scale, flush, info)."""
    return {k: ratio(v, ref[0][k], ref[1][k], ref[2][k]) for k, v in got.items() if v is not None and k in ref[0]}
