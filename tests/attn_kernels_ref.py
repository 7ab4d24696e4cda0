"""The layer-by-layer attention kernels (csrc/attention.hip, csrc/linattn.hip) and the channel LayerNorm (csrc/layernorm.hip) in plain torch on the CPU, fp64, forward
and hand-written backward (no autograd), with an ERROR SCALE per output, built stage by stage as tests/attn_ref.py's docstring describes. Test
infrastructure only. Unlike attn_ref these start from a GIVEN qkv / x (exact fp32 inputs): no LayerNorm or projection in front, so a stage's
scale starts from the rounding of its own terms:

  softmax attention (wdno_attn_fwd / _bwd), on the strided unit / token addressing of wdno_attn_desc, optional rotary tables and bias:
      q' = rot(scale q), k' = rot(k)          s = rot_abs(|.|)                           (0 for k without tables: k is used as given)
      l  = q' k'^T + bias                     s_l = s_q |k'|^T + |q'| s_k^T + |q'| |k'|^T + |bias|
      p  = softmax(l)                         s_p = p (1 + s_l + sum p s_l)
      out = p v                               s_p |v|
      dp = do v^T, delta = sum_j p dp, ds = p (dp - delta)         s_ds = s_p (|dp| + |delta|) + p (s_dp + s_delta)
      dq = scale rot^T(ds k'), dk = rot^T(ds^T q'), dv = p^T do, dbias = sum over the units of ds
  linear attention (wdno_linattn_fwd / _bwd), contiguous units:
      qs = scale softmax_d(q), ks = softmax_n(k)       s = . (1 + a + sum . a), a = |x - max x|: the rounding of the shifted argument
      kstats = (max_n k, sum_n exp(k - max))           the maximum is exact; s_sum = sum exp(k - max) (1 + a + depth)
      ctx = ks^T v, out = qs ctx                       products as above, ctx and dctx with depth x sum |addends| (reference_lin); the
                                                       backward as attn_ref.reference_l from do on
  channel LayerNorm, gain only, dx += add_to          y: xs_h |g|; dx, dg: attn_ref._ln_backward with the xs_h of reference_ln

THE GATE is attn_ref's: |got - ref| <= K 2^-24 scale + flush. flush is one absolute constant, FLUSH = 2^-100: the probabilities of the `sharp`
and `wide` families fall below the smallest normal fp32 number, where a device may flush exp's result to zero; every family keeps max|output|
above 2^-40 (tests/test_host_attn_kernels_ref.py checks it), so the constant is 2^-60 of an output's size and never decides a comparison of
numbers the format resolves.

K, one per output kind, is NOT taken from the kernels. The transcriptions below restate the kernels' arithmetic in fp32 torch -- the softmax with
whole rows ('whole': the one- and two-tile matrix kernels), with an online rescale over 32-key tiles ('tiled') and key by key ('rows': the
thread-per-row kernels, which then recompute p = exp(l - m) (1 / sum)); delta from the saved fp32 forward output (every backward above 32 tokens) or
as sum_j p dp (the matrix kernel up to 32); the bias gradient summed over the units one after the other; the chunked k statistics with
softmax_merge and the chunked context with its merge in chunk order; the two-pass LayerNorm with dg summed row group by row group, then over the
groups of a block, then over the blocks. The worst ratio over the whole matrix (tests/test_host_attn_kernels_ref.py re-measures it and holds it
to K / 2) is

    MEASURED = {a_out: 0.894, a_dqkv: 1.672, a_dbias: 0.544, l_out: 0.334, l_ksum: 0.186, l_ctx: 0.233, l_dqkv: 0.298,
                n_y: 0.471, n_dx: 0.98, n_dg: 0.142}

and K = ceil(4 x that), the project's margin (groupnorm_ref.py: the device's expf and division are a few ulp where the host's are at most 1, FMA
contraction moves single roundings, the order of the sum inside a matrix instruction is not ours to specify):

    K = {a_out: 4, a_dqkv: 7, a_dbias: 3, l_out: 2, l_ksum: 1, l_ctx: 1, l_dqkv: 2, n_y: 2, n_dx: 4, n_dg: 1}
"""
import functools
import math

import torch

from tests.attn_ref import DH, EPS, U, _ln, _ln_backward, _rot, _rot_abs, f32, f64, planes, ratio, rot_tables, scale_from_amax  # noqa: F401  (re-exported)

FLUSH = 2.0 ** -100
SCALE = DH ** -0.5
MEASURED = {'a_out': 0.894, 'a_dqkv': 1.672, 'a_dbias': 0.544, 'l_out': 0.334, 'l_ksum': 0.186, 'l_ctx': 0.233, 'l_dqkv': 0.298,
            'n_y': 0.471, 'n_dx': 0.98, 'n_dg': 0.142}
K = {k: math.ceil(4 * v) for k, v in MEASURED.items()}
KIND = {'attn': {'out': 'a_out', 'dqkv': 'a_dqkv', 'dbias': 'a_dbias'},
        'lin': {'out': 'l_out', 'ksum': 'l_ksum', 'ctx': 'l_ctx', 'dqkv': 'l_dqkv'},
        'ln': {'y': 'n_y', 'dx': 'n_dx', 'dg': 'n_dg'}}
CUS = 256                                    # the compute units the regimes below are stated for (an MI355X; the library's answer without a device)


# ------------------------------------------------------------------------------------------------------------------ softmax attention: cases
def layout(kind, a, b, n, pad=0):
    """(n_uo, n_ui, n_tok, so, si, st, rows) of a unit layout. 'temporal': a samples of b pixels, tokens strided by the pixels (the frames of one
    pixel of CL [a, n, b]); 'spatial': a x b units of n contiguous tokens. pad: rows between two outer units that belong to no unit."""
    if kind == 'temporal':
        so = n * b + pad
        return (a, b, n, so, 1, b, a * so)
    so = b * n + pad
    return (a, b, n, so, n, 1, a * so)


def A(name, lay, heads=4, rot=True, bias=True, dbias=None, bwd=True, debug=0, fam='gauss', grad='gauss', fwd=None, back=None):
    """A softmax-attention case. dbias None: a bias gradient whenever there is a bias and a backward. fwd / back: the entries of ops.attn_plan
    the case exists for."""
    dbias = (bias and bwd) if dbias is None else dbias
    return dict(name=name, lay=lay, heads=heads, rot=rot, bias=bias, dbias=dbias, bwd=bwd, debug=debug, fam=fam, grad=grad, fwd=fwd or {}, back=back or {})


_T, _S = 'temporal', 'spatial'
A_CASES = []
# token counts with rotation and bias: the matrix kernels up to 32 / 64 (forward), the thread-per-row backward above 32; 5 units = 20 items
for _n in (1, 2, 23, 24, 25, 31, 32):
    A_CASES.append(A('rb%d' % _n, layout(_T, 1, 5, _n), fwd=dict(family='mfma24' if _n == 24 else 'mfma', max_walk=1),
                     back=dict(family='mfma24' if _n == 24 else 'mfma', dbias_in_lds=0)))
A_CASES.append(A('rb24-generic', layout(_T, 1, 5, 24), debug=44, fwd=dict(family='mfma'), back=dict(family='mfma')))
for _n, _ipb in ((33, 3), (48, 2), (63, 2), (64, 1), (65, 1), (77, 1)):          # 64: one item per block so that the bias-gradient partial fits (was refused)
    A_CASES.append(A('rb%d' % _n, layout(_T, 1, 5, _n), fwd=dict(family='mfma64' if _n <= 64 else 'rows'),
                     back=dict(family='rows', items_per_block=_ipb, dbias_in_lds=1)))
for _n in (100, 127):                                                             # a bias, no bias gradient
    A_CASES.append(A('rb%d-nodbias' % _n, layout(_T, 1, 3, _n), dbias=False, fwd=dict(family='rows'), back=dict(family='rows', items_per_block=1)))
A_CASES.append(A('rb128-fwd', layout(_T, 1, 3, 128), bwd=False, fwd=dict(family='rows', items_per_block=2)))
# without tables: the tiled forward, the staged / unstaged tiled backward
for _n, _b in ((64, 'big'), (65, 'tiled_staged'), (127, 'tiled_staged'), (128, 'tiled_staged'), (129, 'tiled_unstaged'), (576, 'tiled_unstaged')):
    A_CASES.append(A('plain%d' % _n, layout(_S, 3, 1, _n), rot=False, bias=False, fwd=dict(family='mfma64' if _n <= 64 else 'tiled'), back=dict(family=_b)))
A_CASES.append(A('plain100-ui', layout(_S, 2, 3, 100), rot=False, bias=False, fwd=dict(family='tiled'), back=dict(family='tiled_staged')))
for _n in (577, 1024):
    A_CASES.append(A('plain%d-fwd' % _n, layout(_S, 1, 1, _n), rot=False, bias=False, bwd=False, fwd=dict(family='tiled')))
# item counts: one item, fewer items than a block's waves, exactly the grid cap (4 CUS blocks forward = 4096 items, 3 CUS backward = 3072), one more
A_CASES.append(A('one-item', layout(_T, 1, 1, 24), heads=1, fwd=dict(grid=1), back=dict(grid=1, dbias_in_lds=4)))
A_CASES.append(A('three-items', layout(_S, 3, 1, 7), heads=1, fwd=dict(grid=1), back=dict(grid=1)))
for _n in (2, 24):
    A_CASES.append(A('cap-%d' % _n, layout(_T, 1, 1024, _n), fwd=dict(grid=4 * CUS, max_walk=1), back=dict(grid=3 * CUS, max_walk=2)))
    A_CASES.append(A('cap+1-%d' % _n, layout(_T, 5, 205, _n), fwd=dict(grid=4 * CUS, max_walk=2), back=dict(grid=3 * CUS, max_walk=2)))
A_CASES.append(A('bwdcap-24', layout(_T, 1, 768, 24), fwd=dict(max_walk=1), back=dict(grid=3 * CUS, max_walk=1)))
A_CASES.append(A('tiled-wrap', layout(_S, 257, 1, 100), rot=False, bias=False, bwd=False, fwd=dict(family='tiled', grid=3 * CUS, max_walk=2)))
A_CASES.append(A('big-wrap', layout(_S, 257, 1, 64), rot=False, bias=False, fwd=dict(family='mfma64'), back=dict(family='big', grid=4 * CUS, max_walk=2)))
A_CASES.append(A('tiledbwd-wrap', layout(_S, 129, 1, 65), rot=False, bias=False, fwd=dict(family='tiled'), back=dict(family='tiled_staged', grid=2 * CUS, max_walk=2)))
# the thread-per-row kernels on the matrix kernels' shapes (debug 5: both directions; 67 / 68: forward / backward above 64 tokens), items % ipb != 0
A_CASES.append(A('rows5-24', layout(_T, 1, 3, 24), debug=5, fwd=dict(family='rows', items_per_block=10, grid=2), back=dict(family='rows', items_per_block=4, grid=3)))      # five would fit: at most `heads` with a bias gradient
A_CASES.append(A('rows5-7', layout(_S, 5, 1, 7), heads=2, debug=5, fwd=dict(family='rows', items_per_block=36), back=dict(family='rows', items_per_block=2)))
# ... and a ragged last group in the backward too: five item slots, 12 and 24 items (with a bias gradient a block takes at most `heads` items)
A_CASES.append(A('rows5-24-nodbias', layout(_T, 1, 3, 24), debug=5, dbias=False, fwd=dict(family='rows'), back=dict(family='rows', items_per_block=5, grid=3)))
A_CASES.append(A('rows5-24-h8', layout(_T, 1, 3, 24), heads=8, debug=5, fwd=dict(family='rows'), back=dict(family='rows', items_per_block=5, grid=5, dbias_in_lds=1)))
A_CASES.append(A('rows67-100', layout(_S, 3, 1, 100), rot=False, bias=False, debug=67, fwd=dict(family='rows', items_per_block=2), back=dict(family='tiled_staged')))
A_CASES.append(A('rows68-100', layout(_S, 3, 1, 100), rot=False, bias=False, debug=68, fwd=dict(family='tiled'), back=dict(family='big')))
A_CASES.append(A('rows68-130', layout(_S, 2, 1, 130), rot=False, bias=False, debug=68, fwd=dict(family='tiled'), back=dict(family='big')))
# more than 1024 groups with a bias gradient: the blocks of the thread-per-row backward walk over the groups
A_CASES.append(A('groups-wrap', layout(_T, 1, 770, 33), back=dict(family='rows', items_per_block=3, grid=1024, max_walk=2, dbias_partials=1024)))
# the bias-gradient partial in LDS (heads != 4) and in registers, tables one at a time
for _h in (1, 2, 8):
    A_CASES.append(A('heads%d' % _h, layout(_T, 2, 3, 24), heads=_h, back=dict(family='mfma24', dbias_in_lds=1 if _h % 4 == 0 else 4)))      # a partial per wave
    A_CASES.append(A('heads%d-40' % _h, layout(_T, 1, 3, 40), heads=_h, back=dict(family='rows', dbias_in_lds=1, items_per_block=min(_h, 3))))
A_CASES.append(A('bias-nodbias', layout(_T, 1, 5, 24), dbias=False, back=dict(dbias_partials=0)))
A_CASES.append(A('rot-only', layout(_T, 1, 5, 24), bias=False))
A_CASES.append(A('bias-only', layout(_T, 1, 5, 24), rot=False))
A_CASES.append(A('rot-only-48', layout(_T, 1, 5, 48), bias=False, back=dict(family='rows')))
A_CASES.append(A('spatial-ui-rb', layout(_S, 2, 3, 24)))
# input and gradient families: the matrix kernel, the two-tile forward with the thread-per-row backward, the tiled pair
for _fam, _grad in (('wide', 'gauss'), ('const', 'gauss'), ('sharp', 'gauss'), ('ramp', 'gauss'), ('gauss', 'onehot'), ('gauss', 'spike'), ('wide', 'spike')):
    A_CASES.append(A('f24-%s-%s' % (_fam, _grad), layout(_T, 1, 6, 24), fam=_fam, grad=_grad))
    A_CASES.append(A('f40-%s-%s' % (_fam, _grad), layout(_T, 1, 3, 40), fam=_fam, grad=_grad))
    A_CASES.append(A('f100-%s-%s' % (_fam, _grad), layout(_S, 2, 1, 100), rot=False, bias=False, fam=_fam, grad=_grad))
A_BY_NAME = {c['name']: c for c in A_CASES}
assert len(A_BY_NAME) == len(A_CASES)
# the cases the plane-delivering forms are run on: forward up to 64 tokens (one- and two-tile matrix kernels, a second pass), backward up to 32
PA_FWD = ['rb1', 'rb2', 'rb23', 'rb24', 'rb24-generic', 'rb32', 'rb33', 'rb48', 'rb64', 'one-item', 'cap+1-24', 'heads2', 'rot-only', 'bias-only', 'spatial-ui-rb',
          'f24-wide-gauss', 'f40-wide-gauss', 'f40-sharp-gauss', 'f24-ramp-gauss']
PA_BWD = ['rb1', 'rb2', 'rb23', 'rb24', 'rb24-generic', 'rb32', 'one-item', 'cap-24', 'heads1', 'heads8', 'bias-nodbias', 'rot-only', 'bias-only', 'spatial-ui-rb',
          'f24-wide-gauss', 'f24-sharp-gauss', 'f24-ramp-gauss', 'f24-gauss-onehot', 'f24-gauss-spike', 'f24-wide-spike']


def _gen(salt, *vals):
    return torch.Generator().manual_seed(salt + sum(p * int(v) for p, v in zip((7, 1009, 31, 211, 13, 17, 19, 23), vals)))


def _row_pow(gen, rows, span):
    """a power of two per row, exponents uniform in [-span, span]"""
    return torch.exp2(torch.randint(-span, span + 1, (rows, 1), generator=gen).double())


def _dy_family(dy, grad, gen, tok_of_row, n):
    """dy [rows, width] of a gradient family; tok_of_row: the token index of a row"""
    if grad == 'onehot':
        out = torch.zeros_like(dy)
        out[torch.arange(dy.shape[0]), torch.randint(0, dy.shape[1], (dy.shape[0],), generator=gen)] = 1.0
        return out
    if grad == 'spike':                                                   # large on one token only
        return dy * torch.where(tok_of_row == n // 2, 2.0 ** 10, 1.0)[:, None]
    return dy


@functools.lru_cache(maxsize=4)
def a_inputs(name):
    """fp32 CPU tensors of a softmax-attention case (shared: read-only): qkv [rows, 3 HD], cos / sin [n, 32] | None, bias [heads, n, n] | None,
    dout [rows, HD] | None, idx [units, n] = the row of (unit, token)."""
    c = A_BY_NAME[name]
    n_uo, n_ui, n, so, si, st, rows = c['lay']
    heads, hd = c['heads'], c['heads'] * DH
    gen = _gen(41, n_uo, n_ui, n, heads, len(name))
    r = lambda *s: torch.randn(*s, generator=gen, dtype=f64)
    idx = ((torch.arange(n_uo) * so)[:, None, None] + (torch.arange(n_ui) * si)[None, :, None] + (torch.arange(n) * st)[None, None, :]).reshape(-1, n)
    tok = torch.zeros(rows, dtype=torch.long)
    tok[idx] = torch.arange(n)[None, :].expand_as(idx)
    qkv = r(rows, 3 * hd)
    fam = c['fam']
    if fam == 'wide':                                                     # v over 2^+-12 per row, q and k over 2^+-2 (their product is an exponent)
        qkv[:, :2 * hd] *= _row_pow(gen, rows, 2)
        qkv[:, 2 * hd:] *= _row_pow(gen, rows, 12)
    elif fam == 'const':                                                  # every token of the first and the last unit alike: a uniform softmax without bias
        for u in (0, idx.shape[0] - 1):
            qkv[idx[u]] = qkv[idx[u][0]].clone()
    elif fam == 'sharp':                                                  # one key dominates each row
        qkv[:, hd:2 * hd] *= 6.0
    elif fam == 'ramp':                                                   # first and last token differ in size by 2^6
        qkv *= torch.exp2(6.0 * tok.double() / max(n - 1, 1))[:, None] / 8.0
    out = dict(qkv=qkv, idx=idx, cos=None, sin=None, bias=None, dout=None)
    if c['rot']:
        out['cos'], out['sin'] = rot_tables(1.0 / (10000 ** (torch.arange(0, DH, 2).double() / DH)), n)
    if c['bias']:
        out['bias'] = r(heads, n, n)
    if c['bwd']:
        out['dout'] = _dy_family(r(rows, hd), c['grad'], gen, tok, n)
    return {k: (v.float() if v is not None and v.is_floating_point() else v) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------------------------ softmax attention: fp64
def _units(t, idx, heads):
    """rows [R, k heads 32] -> k tensors [units, heads, n, 32]"""
    g = t[idx]                                                            # [U, n, k HD]
    return [x.reshape(*x.shape[:-1], heads, DH).transpose(-2, -3) for x in g.chunk(g.shape[-1] // (heads * DH), -1)]


def _rows(parts, idx, rows, like=None):
    """the inverse: [units, heads, n, 32] tensors -> rows [R, k HD]; rows of no unit are zero (or `like`'s)"""
    g = torch.cat([p.transpose(-2, -3).reshape(*p.shape[:1], p.shape[-2], -1) for p in parts], -1)
    out = torch.zeros(rows, g.shape[-1], dtype=g.dtype) if like is None else like.clone()
    out[idx] = g
    return out


def reference_attn(qkv, idx, heads, cos=None, sin=None, bias=None, dout=None, scale=SCALE):
    """fp64 outputs and scales of softmax attention: ({out, dqkv, dbias}, {the same: scale}) as row tensors (dbias [heads, n, n])."""
    rows, n = qkv.shape[0], idx.shape[1]
    q, k, v = _units(qkv.double(), idx, heads)
    q = q * scale
    s_q, s_k = q.abs(), torch.zeros_like(k)
    if cos is not None:
        cos, sin = cos.double(), sin.double()
        s_q, s_k = _rot_abs(q.abs(), cos, sin), _rot_abs(k.abs(), cos, sin)
        q, k = _rot(q, cos, sin), _rot(k, cos, sin)
    kt = k.transpose(-1, -2)
    lg = q @ kt
    s_lg = s_q @ kt.abs() + q.abs() @ s_k.transpose(-1, -2) + q.abs() @ kt.abs()
    if bias is not None:
        lg, s_lg = lg + bias.double(), s_lg + bias.double().abs()
    p = torch.softmax(lg, -1)
    s_p = p * (1 + s_lg + (p * s_lg).sum(-1, keepdim=True))
    o, s_o = p @ v, s_p @ v.abs()
    out, sc = {'out': _rows([o], idx, rows)}, {'out': _rows([s_o], idx, rows)}
    if dout is None:
        return out, sc
    do, = _units(dout.double(), idx, heads)
    vt, pt = v.transpose(-1, -2), p.transpose(-1, -2)
    dp, s_dp = do @ vt, do.abs() @ vt.abs()
    dv, s_dv = pt @ do, s_p.transpose(-1, -2) @ do.abs()
    delta = (p * dp).sum(-1, keepdim=True)
    s_delta = (s_p * dp.abs() + p * s_dp).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    s_ds = s_p * (dp.abs() + delta.abs()) + p * (s_dp + s_delta)
    if bias is not None:
        out['dbias'], sc['dbias'] = ds.sum(0), s_ds.sum(0)
    dst = ds.transpose(-1, -2)
    dq, s_dq = ds @ k, s_ds @ k.abs() + ds.abs() @ s_k
    dk, s_dk = dst @ q, s_ds.transpose(-1, -2) @ q.abs() + dst.abs() @ s_q
    if cos is not None:
        dq, s_dq, dk, s_dk = _rot(dq, cos, sin, True), _rot_abs(s_dq, cos, sin), _rot(dk, cos, sin, True), _rot_abs(s_dk, cos, sin)
    out['dqkv'], sc['dqkv'] = _rows([dq * scale, dk, dv], idx, rows), _rows([s_dq * scale, s_dk, s_dv], idx, rows)
    return out, sc


@functools.lru_cache(maxsize=4)
def reference_of_a(name):
    t, c = a_inputs(name), A_BY_NAME[name]
    return reference_attn(t['qkv'], t['idx'], c['heads'], t['cos'], t['sin'], t['bias'], t['dout'])


def softmax_form(family):
    """how a kernel family of ops.attn_plan forms its softmax (module docstring)"""
    return {'mfma24': 'whole', 'mfma': 'whole', 'mfma64': 'whole', 'tiled': 'tiled', 'tiled_staged': 'tiled', 'tiled_unstaged': 'tiled', 'big': 'rows',
            'rows': 'rows'}[family]


def _stats32(lg, tile):
    """running (max, sum exp) of fp32 logits over key tiles of `tile` keys, as the kernels rescale them"""
    m = torch.full(lg.shape[:-1] + (1,), -math.inf)
    l = torch.zeros_like(m)
    for j0 in range(0, lg.shape[-1], tile):
        s = lg[..., j0:j0 + tile]
        mn = torch.maximum(m, s.amax(-1, keepdim=True))
        l = l * torch.exp(m - mn) + torch.exp(s - mn).sum(-1, keepdim=True)
        m = mn
    return m, l


def transcription_attn(qkv, idx, heads, cos=None, sin=None, bias=None, dout=None, scale=SCALE, form='whole', form_bwd='rows', delta_from_out=True):
    """The kernels' arithmetic in fp32 torch; {name: fp32 tensor} like reference_attn."""
    rows, n = qkv.shape[0], idx.shape[1]
    q, k, v = _units(qkv.float(), idx, heads)
    q = q * scale
    if cos is not None:
        cos, sin = cos.float(), sin.float()
        q, k = _rot(q, cos, sin), _rot(k, cos, sin)
    lg = q @ k.transpose(-1, -2)
    if bias is not None:
        lg = lg + bias.float()

    def probs(kind):
        if kind == 'whole':
            e = torch.exp(lg - lg.amax(-1, keepdim=True))
            return e * (1.0 / e.sum(-1, keepdim=True))
        m, l = _stats32(lg, 32 if kind == 'tiled' else 1)
        return torch.exp(lg - m) * (1.0 / l)
    if form == 'tiled':                                                   # the accumulator is rescaled with the running maximum and divided at the end
        m = torch.full(lg.shape[:-1] + (1,), -math.inf)
        l, acc = torch.zeros_like(m), torch.zeros_like(q)
        for j0 in range(0, n, 32):
            s = lg[..., j0:j0 + 32]
            mn = torch.maximum(m, s.amax(-1, keepdim=True))
            f, e = torch.exp(m - mn), torch.exp(s - mn)
            l, acc, m = l * f + e.sum(-1, keepdim=True), acc * f + e @ v[..., j0:j0 + 32, :], mn
        o = acc * (1.0 / l)
    else:
        o = probs(form) @ v
    out = {'out': _rows([o], idx, rows)}
    if dout is None:
        return out
    do, = _units(dout.float(), idx, heads)
    p = probs(form_bwd)
    dp = do @ v.transpose(-1, -2)
    delta = (do * o).sum(-1, keepdim=True) if delta_from_out else (p * dp).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    if bias is not None:
        out['dbias'] = ds.cumsum(0)[-1]                                       # one unit after the other
    dq, dk, dv = ds @ k, ds.transpose(-1, -2) @ q, p.transpose(-1, -2) @ do
    if cos is not None:
        dq, dk = _rot(dq, cos, sin, True), _rot(dk, cos, sin, True)
    out['dqkv'] = _rows([dq * scale, dk, dv], idx, rows)
    return out


# ------------------------------------------------------------------------------------------------------------------ linear attention
def L(name, units, n, heads=4, bwd=True, debug=0, fam='gauss', grad='gauss', plan=None, plan_bwd=None):
    return dict(name=name, units=units, n=n, heads=heads, bwd=bwd, debug=debug, fam=fam, grad=grad, plan=plan or {}, plan_bwd=plan_bwd or {})


L_CASES = []
for _n, _ks, _cc, _tt in ((1, 1, 1, 1), (31, 1, 1, 1), (32, 1, 1, 1), (33, 1, 1, 1), (63, 1, 1, 1), (64, 1, 1, 1), (127, 1, 1, 1), (128, 2, 1, 1), (129, 2, 1, 2),
                          (255, 3, 1, 2), (256, 4, 2, 2), (1000, 15, 7, 8), (1024, 16, 8, 8), (2053, 16, 16, 17)):
    L_CASES.append(L('n%d' % _n, 2, _n, plan=dict(kstats_chunks=_ks, ctx_chunks=_cc, token_tiles=_tt, family='mfma'), plan_bwd=dict(ctx_chunks=_cc)))
for _h in (1, 2):
    L_CASES.append(L('h%d-n33' % _h, 3, 33, heads=_h))
    L_CASES.append(L('h%d-n300' % _h, 2, 300, heads=_h, plan=dict(kstats_chunks=4, ctx_chunks=2)))
# one head, n_tok = 128 k, as many context chunks as the token count allows: the chunk partials fill the most of what they alias (out, the hi plane)
for _n, _ks, _cc in ((128, 2, 1), (256, 4, 2), (1024, 16, 8)):
    L_CASES.append(L('h1-n%d' % _n, 2, _n, heads=1, plan=dict(kstats_chunks=_ks, ctx_chunks=_cc, token_tiles=_n // 128), plan_bwd=dict(ctx_chunks=_cc)))
# units x heads: 1, just at 2 CUS = 512 (the backward's chunk partials still have their workspace), just over (they do not), far over (one chunk anyway)
L_CASES.append(L('uh1', 1, 260, heads=1, plan=dict(ctx_chunks=2), plan_bwd=dict(ctx_chunks=2)))
L_CASES.append(L('uh512', 128, 256, plan=dict(ctx_chunks=1), plan_bwd=dict(ctx_chunks=1)))
L_CASES.append(L('uh256', 64, 256, plan=dict(ctx_chunks=2), plan_bwd=dict(ctx_chunks=2)))
L_CASES.append(L('uh516', 129, 256, plan=dict(ctx_chunks=1), plan_bwd=dict(ctx_chunks=1)))
L_CASES.append(L('uh2000', 500, 130, plan=dict(ctx_chunks=1), plan_bwd=dict(ctx_chunks=1)))
for _n in (33, 129, 300):
    L_CASES.append(L('tok5-n%d' % _n, 3, _n, debug=5, plan=dict(family='tokens', token_tiles=-(-_n // 64))))
L_CASES.append(L('tok5-h1', 3, 70, heads=1, debug=5, plan=dict(family='tokens')))
for _fam, _grad in (('wide', 'gauss'), ('const', 'gauss'), ('sharp', 'gauss'), ('ramp', 'gauss'), ('gauss', 'onehot'), ('gauss', 'spike'), ('wide', 'spike')):
    L_CASES.append(L('f300-%s-%s' % (_fam, _grad), 2, 300, fam=_fam, grad=_grad))
    L_CASES.append(L('f40-%s-%s' % (_fam, _grad), 3, 40, fam=_fam, grad=_grad))
L_BY_NAME = {c['name']: c for c in L_CASES}
assert len(L_BY_NAME) == len(L_CASES)
PL = ['h1-n128', 'h1-n256', 'h1-n1024', 'n1', 'n33', 'n128', 'n129', 'n2053', 'h2-n300', 'uh516', 'f300-wide-gauss', 'f300-sharp-gauss', 'f300-ramp-gauss', 'f300-gauss-onehot',
      'f300-wide-spike', 'f40-const-gauss']


@functools.lru_cache(maxsize=4)
def l_inputs(name):
    """fp32 CPU tensors of a linear-attention case: qkv [units n, 3 HD], dout [units n, HD] | None"""
    c = L_BY_NAME[name]
    units, n, hd = c['units'], c['n'], c['heads'] * DH
    gen = _gen(53, units, n, c['heads'], len(name))
    r = lambda *s: torch.randn(*s, generator=gen, dtype=f64)
    rows = units * n
    tok = torch.arange(rows) % n
    qkv = r(rows, 3 * hd)
    fam = c['fam']
    if fam == 'wide':                                                     # v over 2^+-12 per row, q and k (exponents) over 2^+-2
        qkv[:, :2 * hd] *= _row_pow(gen, rows, 2)
        qkv[:, 2 * hd:] *= _row_pow(gen, rows, 12)
    elif fam == 'const':                                                  # the first unit: every token alike (a uniform softmax over the tokens)
        qkv[:n] = qkv[0].clone()
    elif fam == 'sharp':                                                  # one token dominates each column of k, one channel each row of q
        qkv[:, :2 * hd] *= 6.0
    elif fam == 'ramp':                                                   # k grows along the tokens: every chunk raises the running maximum
        qkv[:, hd:2 * hd] += (8.0 * tok.double() / max(n - 1, 1))[:, None]
        qkv[:, 2 * hd:] *= torch.exp2(6.0 * tok.double() / max(n - 1, 1))[:, None] / 8.0
    dout = _dy_family(r(rows, hd), c['grad'], gen, tok, n) if c['bwd'] else None
    return dict(qkv=qkv.float(), dout=None if dout is None else dout.float())


def _lheads(t, units, n, heads):
    g = t.reshape(units, n, -1)
    return [x.reshape(units, n, heads, DH).transpose(1, 2) for x in g.chunk(g.shape[-1] // (heads * DH), -1)]


def _lrows(parts):
    return torch.cat([p.transpose(1, 2).reshape(p.shape[0] * p.shape[2], -1) for p in parts], -1)


def k_depth(n, heads, chunks):
    """roundings one addend of the k statistics' sum meets at most: a row group (256 / HD of them per block) adds its share of a chunk's rows
    one by one, then the groups and the chunks are merged in order"""
    nrg = 256 // (heads * DH)
    return -(-(-(-n // chunks)) // nrg) + nrg + chunks


def ctx_depth(n, chunks):
    """... and of the context's sum over the tokens: a wave adds every fourth token pair of its chunk (rounded up to 8 tokens) in turn on
    the matrix unit, then the four waves and the chunks are added"""
    return -(-((-(-n // chunks) + 7) & ~7) // 8) + 2 + chunks


def reference_lin(qkv, units, n, heads, dout=None, scale=SCALE, kstats_chunks=1, ctx_chunks=1, ctx_chunks_bwd=1):
    """fp64 outputs and scales of linear attention: out [rows, HD], kmax / ksum [units, HD], ctx [units, heads, 32, 32], dqkv [rows, 3 HD].
    The sums over the tokens are LONG and not random walks on every family (equal addends: the `const` rows; one dominant addend: `sharp`), so
    their scales carry the first-order bound of a sequential sum, (roundings an addend meets) x sum |addends|, with the depth the cuts
    ops.linattn_plan reports give (k_depth, ctx_depth)."""
    q, k, v = _lheads(qkv.double(), units, n, heads)                      # [U, h, n, 32]
    dk_, dc_, dcb_ = k_depth(n, heads, kstats_chunks), ctx_depth(n, ctx_chunks), ctx_depth(n, ctx_chunks_bwd)
    a_q = (q - q.amax(-1, keepdim=True)).abs()
    sm = torch.softmax(q, -1)
    qs = sm * scale
    s_qs = qs * (1 + a_q + (sm * a_q).sum(-1, keepdim=True))
    kmax = k.amax(-2, keepdim=True)
    a_k = (k - kmax).abs()
    e = torch.exp(k - kmax)
    ksum = e.sum(-2, keepdim=True)
    ks = e / ksum
    s_ks = ks * (1 + a_k + (ks * a_k).sum(-2, keepdim=True) + dk_)
    kst = ks.transpose(-1, -2)
    ctx, s_ctx = kst @ v, s_ks.transpose(-1, -2) @ v.abs() + dc_ * (kst @ v.abs())
    o, s_o = qs @ ctx, s_qs @ ctx.abs() + qs @ s_ctx
    out = {'out': _lrows([o]), 'kmax': kmax.reshape(units, -1), 'ksum': ksum.reshape(units, -1), 'ctx': ctx}
    sc = {'out': _lrows([s_o]), 'ksum': (e * (1 + a_k + dk_)).sum(-2).reshape(units, -1), 'ctx': s_ctx}
    if dout is None:
        return out, sc
    do, = _lheads(dout.double(), units, n, heads)
    qst = qs.transpose(-1, -2)
    dctx, s_dctx = qst @ do, s_qs.transpose(-1, -2) @ do.abs() + dcb_ * (qst @ do.abs())
    ctxt = ctx.transpose(-1, -2)
    dqs, s_dqs = do @ ctxt, do.abs() @ s_ctx.transpose(-1, -2)
    inner = (qs * dqs).sum(-1, keepdim=True) / scale
    s_inner = (s_qs * dqs.abs() + qs * s_dqs).sum(-1, keepdim=True) / scale
    dq = qs * (dqs - inner)
    s_dq = s_qs * (dqs.abs() + inner.abs()) + qs * (s_dqs + s_inner)
    dctxt = dctx.transpose(-1, -2)
    dks, s_dks = v @ dctxt, v.abs() @ s_dctx.transpose(-1, -2)
    T = (dctx * ctx).sum(-1)[..., None, :]
    s_T = (s_dctx * ctx.abs() + dctx.abs() * s_ctx).sum(-1)[..., None, :]
    dk = ks * (dks - T)
    s_dk = s_ks * (dks.abs() + T.abs()) + ks * (s_dks + s_T)
    dv, s_dv = ks @ dctx, s_ks @ dctx.abs() + ks @ s_dctx
    out['dqkv'], sc['dqkv'] = _lrows([dq, dk, dv]), _lrows([s_dq, s_dk, s_dv])
    return out, sc


@functools.lru_cache(maxsize=4)
def reference_of_l(name, cuts=(1, 1, 1)):
    """cuts: (kstats_chunks, ctx_chunks, ctx_chunks of the backward) as ops.linattn_plan reports them"""
    t, c = l_inputs(name), L_BY_NAME[name]
    return reference_lin(t['qkv'], c['units'], c['n'], c['heads'], t['dout'], SCALE, *cuts)


def _merge32(m, l, m2, l2):
    """softmax_merge of csrc/linattn.hip"""
    mn = torch.maximum(m, m2)
    a = torch.where(torch.isinf(m), torch.zeros_like(l), l * torch.exp(m - mn))
    b = torch.where(torch.isinf(m2), torch.zeros_like(l2), l2 * torch.exp(m2 - mn))
    return mn, a + b


def _kstats32(k, heads, chunks):
    """linattn_kstats_kernel + linattn_kstats_merge_kernel (csrc/linattn.hip) on k [U, h, n, 32]: (max, sum) [U, h, 32] each. A chunk's rows go round-robin to
    256 / HD row groups, each takes eight rows per round with one rescale per round; groups, then chunks, merge in order."""
    n = k.shape[2]
    nrg = 256 // (heads * DH)
    per = -(-n // chunks)
    M = torch.full(k.shape[:2] + (DH,), -math.inf)
    Lsum = torch.zeros_like(M)
    for c in range(chunks):
        jb, je = c * per, min(n, (c + 1) * per)
        cm, cl = torch.full_like(M, -math.inf), torch.zeros_like(M)
        for rg in range(nrg):
            m, l = torch.full_like(M, -math.inf), torch.zeros_like(M)
            mine = k[:, :, jb + rg:je:nrg] if jb + rg < je else k[:, :, 0:0]
            for r0 in range(0, mine.shape[2], 8):
                vch = mine[:, :, r0:r0 + 8]
                mn = torch.maximum(m, vch.amax(2))
                add = torch.zeros_like(l)
                for u in range(vch.shape[2]):
                    add = add + torch.exp(vch[:, :, u] - mn)
                l = torch.where(torch.isinf(m), torch.zeros_like(l), l * torch.exp(m - mn)) + add
                m = mn
            cm, cl = (m, l) if rg == 0 else _merge32(cm, cl, m, l)
        M, Lsum = _merge32(M, Lsum, cm, cl)
    return M, Lsum


def _chunk_sum32(a, b, chunks):
    """sum_n a[n][d] b[n][e] as linattn_ctx_kernel (csrc/linattn.hip) cuts it: pieces of ((n / chunks rounded up) rounded up to 8) tokens, added in chunk order"""
    n = a.shape[2]
    clen = (-(-n // chunks) + 7) & ~7
    tot = None
    for c in range(chunks):
        t0, t1 = c * clen, min(n, (c + 1) * clen)
        part = torch.zeros(a.shape[:2] + (4, DH, DH))                      # one accumulator per wave: token pairs 2 w, 2 w + 1 of every 8
        for j0 in range(t0, t1, 8):
            aa, bb = torch.zeros(a.shape[:2] + (8, DH)), torch.zeros(a.shape[:2] + (8, DH))
            aa[:, :, :min(8, t1 - j0)], bb[:, :, :min(8, t1 - j0)] = a[:, :, j0:j0 + 8][:, :, :t1 - j0], b[:, :, j0:j0 + 8][:, :, :t1 - j0]
            aa, bb = aa.reshape(*a.shape[:2], 4, 2, DH), bb.reshape(*a.shape[:2], 4, 2, DH)
            part = part + (aa[..., 0, :, None] * bb[..., 0, None, :] + aa[..., 1, :, None] * bb[..., 1, None, :])
        part = (part[:, :, 0] + part[:, :, 1]) + (part[:, :, 2] + part[:, :, 3])
        tot = part if chunks == 1 else (torch.zeros_like(part) + part if tot is None else tot + part)
    return tot


def transcription_lin(qkv, units, n, heads, dout=None, scale=SCALE, kstats_chunks=1, ctx_chunks=1, ctx_chunks_bwd=1):
    """The kernels' arithmetic in fp32 torch, with the cuts ops.linattn_plan reports."""
    q, k, v = _lheads(qkv.float(), units, n, heads)
    M, Lsum = _kstats32(k, heads, kstats_chunks)
    ks = torch.exp(k - M[:, :, None, :]) * (1.0 / Lsum)[:, :, None, :]
    ctx = _chunk_sum32(ks, v, ctx_chunks)
    e = torch.exp(q - q.amax(-1, keepdim=True))
    qs = e * (scale / e.sum(-1, keepdim=True))
    o = qs @ ctx
    out = {'out': _lrows([o]), 'kmax': M.reshape(units, -1), 'ksum': Lsum.reshape(units, -1), 'ctx': ctx}
    if dout is None:
        return out
    do, = _lheads(dout.float(), units, n, heads)
    qs2 = scale * e / e.sum(-1, keepdim=True)                             # the context kernel's form of the same factor
    dctx = _chunk_sum32(qs2, do, ctx_chunks_bwd)
    out['dctx'] = dctx                                                    # (the planes form measures its maximum for the scale bound)
    T = (dctx * ctx).cumsum(-1)[..., -1][..., None, :]
    dqs = do @ ctx.transpose(-1, -2)
    inner = (qs * dqs).sum(-1, keepdim=True) * (1.0 / scale)
    dq = qs * (dqs - inner)
    dk = ks * (v @ dctx.transpose(-1, -2) - T)
    dv = ks @ dctx
    out['dqkv'] = _lrows([dq, dk, dv])
    return out


# ------------------------------------------------------------------------------------------------------------------ channel LayerNorm
LN_C = (4, 8, 12, 16, 32, 36, 64, 96, 128, 256, 260, 512, 516, 1024)      # 32: the only 8-lanes-per-row count (20 .. 32 channels)


def ln_shape(c):
    """(threads per row, float4 per lane) of csrc/layernorm.hip's ln_shape, for the cases' row counts; the GPU test asserts them from the plan"""
    c4 = c // 4
    p2 = lambda v: 1 << (v - 1).bit_length()
    return (max(p2(c4), 2), 1) if c4 <= 64 else (64, p2(-(-c4 // 64)))


def N(c, p, add=True, fam='gauss', grad='gauss', walk=1):
    return dict(name='c%d-p%d-%s-%s-%s' % (c, p, 'add' if add else 'noadd', fam, grad), c=c, p=p, add=add, fam=fam, grad=grad, walk=walk)


N_CASES = []
for _c in LN_C:
    _rpb = 256 // ln_shape(_c)[0]
    for _p in sorted({1, max(_rpb - 1, 1), _rpb + 1}):
        N_CASES.append(N(_c, _p, add=True))
        N_CASES.append(N(_c, _p, add=False))
N_CASES.append(N(1024, 1024 * 4 + 3, walk=2))                                  # 64 lanes per row: the fewest rows (4 per block) that wrap 1024 blocks
N_CASES.append(N(16, 1024 * 64 + 3, add=False, walk=2))                        # ... and the most rows per block that do
for _fam, _grad in (('wide', 'gauss'), ('const', 'gauss'), ('ramp', 'gauss'), ('gauss', 'onehot'), ('gauss', 'spike'), ('wide', 'spike')):
    N_CASES.append(N(64, 300, fam=_fam, grad=_grad))
    N_CASES.append(N(260, 37, add=False, fam=_fam, grad=_grad))
N_BY_NAME = {c['name']: c for c in N_CASES}
assert len(N_BY_NAME) == len(N_CASES)


@functools.lru_cache(maxsize=4)
def n_inputs(name):
    """fp32 CPU tensors of a LayerNorm case: x [P, C], g [C], dy [P, C], add [P, C] | None"""
    c = N_BY_NAME[name]
    p, ch = c['p'], c['c']
    gen = _gen(67, p, ch, len(name))
    r = lambda *s: torch.randn(*s, generator=gen, dtype=f64)
    x = r(p, ch) * 1.5 + 0.2
    row = torch.arange(p)
    if c['fam'] == 'wide':
        x *= _row_pow(gen, p, 12)
    elif c['fam'] == 'const':                                             # zero variance: the first, a middle and the last row
        for i in sorted({0, p // 2, p - 1}):
            x[i] = x[i, 0].clone()
    elif c['fam'] == 'ramp':
        x *= torch.exp2(6.0 * row.double() / max(p - 1, 1))[:, None] / 8.0
    dy = _dy_family(r(p, ch), c['grad'], gen, row, p)
    return dict(x=x.float(), g=(1 + 0.3 * r(ch)).float(), dy=dy.float(), add=r(p, ch).float() if c['add'] else None)


def ln_depth(c):
    """roundings an addend of a row sum meets at most: a lane adds its 4 x vpl values, then log2(tpr) butterfly steps"""
    tpr, vpl = ln_shape(c)
    return 4 * vpl + tpr.bit_length() - 1


def reference_ln(x, g, dy=None, add=None):
    """fp64 outputs and scales of the channel LayerNorm: y; with dy: dx (+ add), dg. The row sums (mean, variance, the two of the backward) are
    not random walks on every family (a `const` row: equal addends, and y = 0 exactly), so they enter with the first-order bound of their
    summation tree, depth x sum |addends|: xs_h = (|x| + depth mean|x|) rstd + depth |xh|, the second term the variance's share through rstd."""
    xd, gd = x.double(), g.double()
    d = ln_depth(x.shape[-1])
    xh, rstd, mean, _ = _ln(xd, gd)
    xs_h = (xd.abs() + d * xd.abs().mean(-1, keepdim=True)) * rstd + d * xh.abs()
    out, sc = {'y': xh * gd}, {'y': xs_h * gd.abs()}
    if dy is None:
        return out, sc
    dyd = dy.double()
    zero = torch.zeros_like(xd)
    o_, s_, _ = _ln_backward(dyd, d * dyd.abs(), zero, xh, xs_h, rstd, gd, zero if add is None else add.double())
    out.update(dx=o_['dx'], dg=o_['dg'].sum(0))
    sc.update(dx=s_['dx'], dg=s_['dg'].sum(0))
    return out, sc


@functools.lru_cache(maxsize=4)
def reference_of_n(name):
    t = n_inputs(name)
    return reference_ln(t['x'], t['g'], t['dy'], t['add'])


def transcription_ln(x, g, dy=None, add=None, rows_per_block=1, blocks=1):
    """layernorm_kernel's arithmetic in fp32 torch; the launch shape (ops.layernorm_plan) fixes the order of the dg sum: a row group adds its rows
    pass by pass, a block its groups in order, partial_rows_sum the blocks."""
    p, c = x.shape
    x, g = x.float(), g.float()
    mean = x.sum(-1, keepdim=True) * (1.0 / c)
    xc = x - mean
    rstd = 1.0 / torch.sqrt((xc * xc).sum(-1, keepdim=True) * (1.0 / c) + EPS)
    out = {'y': xc * rstd * g}
    if dy is None:
        return out
    dy = dy.float()
    xh = xc * rstd
    dn = dy * g
    m1 = dn.sum(-1, keepdim=True) * (1.0 / c)
    m2 = (dn * xh).sum(-1, keepdim=True) * (1.0 / c)
    dx = rstd * (dn - m1 - xh * m2)
    out['dx'] = dx if add is None else dx + add.float()
    per = blocks * rows_per_block
    passes = -(-p // per)
    dgr = torch.zeros(passes * per, c)
    dgr[:p] = dy * xh
    dgr = dgr.reshape(passes, blocks, rows_per_block, c)
    out['dg'] = dgr.cumsum(0)[-1].cumsum(1)[:, -1].double().sum(0).float()      # partial_rows_sum adds the blocks in fp64
    return out


# ------------------------------------------------------------------------------------------------------------------ the plane-delivering forms
# A tensor delivered as planes is (hi, lo) = (fp16(t s), fp16(t s - hi)) at ONE power-of-two scale s = scale_from_amax(bound), the bound an
# analytic one of max|t| that the kernel forms in fp32 from the amax records of its inputs (csrc/attention.hip and csrc/linattn.hip state each next to the code):
#   softmax attention forward    |out|  <= A                                        (rows of P sum to 1; A = max|qkv|)
#   softmax attention backward   |dqkv| <= 1.01 max(n G, 1.4143 scale n 64 G A^2)   (G = max|dout|)
#   linear attention forward     |out|  <= 1.01 scale A
#   linear attention backward    |dqkv| <= 1.01 max(64 scale A G, 64 A D, 32 D)     (D = max|dctx|, measured by the call)
# The functions below repeat that fp32 arithmetic operation by operation, so that the delivered scale can be compared for equality.
def _f32(x):
    import numpy as np
    return np.float32(x)


def attn_fwd_plane_bound(a):
    return float(_f32(a))


def attn_bwd_plane_bound(n, a, g, scale=SCALE):
    a, g = _f32(a), _f32(g)
    return float(_f32(1.01) * max(_f32(n) * g, _f32(1.4143) * _f32(scale) * _f32(n) * _f32(64) * g * a * a))


def lin_fwd_plane_bound(a, scale=SCALE):
    return float(_f32(1.01) * _f32(scale) * _f32(a))


def lin_bwd_plane_bound(a, g, d, scale=SCALE):
    a, g, d = _f32(a), _f32(g), _f32(d)
    return float(_f32(1.01) * max(_f32(64) * _f32(scale) * a * g, max(_f32(64) * a * d, _f32(32) * d)))


def plane_ratio(hi, lo, s, ref, scale, k):
    """A plane pair against the fp64 reference: max of (|(hi + lo) / s - ref| - the split's own rounding) / (k 2^-24 scale). The split: the lo
    plane carries 11 bits below the hi plane's 11 (2^-22 |ref|) and is sub-normal below 2^-14 (half a step of 2^-24: 2^-25 / s)."""
    err = ((hi.double() + lo.double()) / s - ref).abs() - 2.0 ** -22 * ref.abs() - 2.0 ** -25 / s - FLUSH
    return float((err.clamp_min(0) / (k * U * scale).clamp_min(1e-300)).max())


def bf16_ratio(got, ref, scale, k):
    """The single bf16 plane, in units of 2^-9: bf16 keeps 8 significant bits, round to nearest is off by half a step, a step is at most 2^-7 of
    the value rounded (which is the reference up to the gate): 2 units, 2^-8 (|ref| + k 2^-24 scale), on top of the gate; 2^-126 for the
    sub-normal values a device may flush."""
    gate = k * U * scale
    err = (got.double() - ref).abs() - 2 * 2.0 ** -9 * (ref.abs() + gate) - 2.0 ** -126
    return float((err.clamp_min(0) / gate.clamp_min(1e-300)).max())
