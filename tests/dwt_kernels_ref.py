"""fp64 reference, error scale and case matrix for the wavelet kernels (csrc/dwt.hip, csrc/dwt_analysis.hip, csrc/dwt_synthesis.hip).

REFERENCE. Plain numpy, written from the two formulas at the top of csrc/dwt.hip and from no kernel:
    analysis : y_b[k] = sum_m f_b[L-1-m] X(2k + m - off)                                    (b = lo, hi)
    synthesis: x[n]   = sum_{m : (n+off-m) even} lo[K] g_lo[m] + hi[K] g_hi[m],  K = (n+off-m)/2
with off = L - 2 and zero extension (mode 'zero'), or off = L/2 - 1 and periodic extension (mode 'per'; an odd length is extended by repeating
its last sample, and in the adjoint of that analysis the sample of the repeated position N is folded back onto N - 1). The four entry points are
compositions of the two primitives over the transformed axes (analysis T, H, W; synthesis W, H, T): fwd = analysis with the decomposition pair,
inv = synthesis with the reconstruction pair, inv_adjoint = analysis with the reversed reconstruction pair, fwd_adjoint = synthesis with the
reversed decomposition pair. Band order: 3-D bt 4 + bh 2 + bw, 2-D bw 2 + bh, 1-D bw. The coefficient tensor may be strided
(coef_strides / coef_offsets), and packed_* is the layout of wdno_dwt_fwd_packed. Taps enter as the fp32 values the library receives.
The primitives run in the dtype they are given: float64 is the reference, float32 (every product and every add rounded, no fma: the worse case)
is the TRANSCRIPTION that shows the gate holds for a correct fp32 implementation (tests/test_host_dwt_kernels_ref.py).

SCALE AND GATE. S_e = the same transform of |input| with |taps| in fp64; |got - ref| <= K 2^-24 S_e with K = nd (L + 1) + 1 (one more for the
division of the packed analysis): the forward bound of nd chained L-term dot products -- L roundings per pass, one more for the fold-back add of
an odd adjoint, one for second-order terms. Derived, not measured on the kernels. Where S_e = 0 the result must be exactly 0.

CASES. Every case names the launch regime it exists for and states, per entry point, what ops.dwt_plan must report (`expect`); the shapes are the
smallest that reach it. REQUIRED is what the matrix as a whole must reach (tests/test_gpu_dwt_matrix.py::test_coverage): every kernel
instantiation the choosers can launch, and both block-count classes (a multiple of 8 -- the only case where xcd_tile renumbers the tiles -- and
not) for every fused family. UNREACHABLE lists the instantiations no shape can launch, with the chooser's arithmetic."""
import itertools

import numpy as np

from wdno_amd.filters import FILTER_BANKS

U = 2.0 ** -24
ENTRIES = ('fwd', 'inv', 'inv_adjoint', 'fwd_adjoint')
ANALYSIS_SHAPED = ('fwd', 'inv_adjoint')
MODE_ID = {'per': 0, 'zero': 1}
FUSED_L = (2, 4, 6, 8, 10)
ALL_L = (2, 4, 6, 8, 10, 12, 14, 16)
DBG_PER_AXIS_DWT = 11          # wdno_amd/csrc/debug_modes.h
DBG_DWT3_SYNTH_LDS = 45
SENTINEL = -7.25


def coef_len(n, L, mode):
    return (n + 1) // 2 if mode == 'per' else (n + L - 1) // 2


def natural_len(m, L, mode):
    return 2 * m if mode == 'per' else 2 * m - L + 2


def gate_k(nd, L, packed=False):
    return nd * (L + 1) + 1 + (1 if packed else 0)


# ------------------------------------------------------------------------------------------------------------------ the two primitives
def analysis_1axis(x, f_lo, f_hi, mode, axis, odd_rule=True):
    """(lo, hi) along `axis`, in the dtype of x; terms in the order m = 0 .. L - 1, product then add."""
    x = np.moveaxis(x, axis, -1)
    dt = x.dtype
    f_lo, f_hi = np.asarray(f_lo, dt), np.asarray(f_hi, dt)
    L, N = len(f_lo), x.shape[-1]
    M = coef_len(N, L, mode)
    k = np.arange(M)
    lo = np.zeros(x.shape[:-1] + (M,), dt)
    hi = np.zeros(x.shape[:-1] + (M,), dt)
    off = L - 2 if mode == 'zero' else L // 2 - 1
    period = N + (N & 1 if odd_rule else 0)
    for m in range(L):
        j = 2 * k + m - off
        if mode == 'zero':
            v = np.where((j >= 0) & (j < N), x[..., np.clip(j, 0, N - 1)], dt.type(0))
        else:
            v = x[..., np.minimum(j % period, N - 1)]              # the repeated last sample of an odd length
        lo = lo + f_lo[L - 1 - m] * v
        hi = hi + f_hi[L - 1 - m] * v
    return np.moveaxis(lo, -1, axis), np.moveaxis(hi, -1, axis)


def synthesis_1axis(lo, hi, g_lo, g_hi, mode, N, axis, odd=False):
    """N samples along `axis` from (lo, hi); odd: the adjoint of a periodized analysis of odd length N (position N folds onto N - 1)."""
    lo, hi = np.moveaxis(lo, axis, -1), np.moveaxis(hi, axis, -1)
    dt = lo.dtype
    g_lo, g_hi = np.asarray(g_lo, dt), np.asarray(g_hi, dt)
    L, M = len(g_lo), lo.shape[-1]
    off = L - 2 if mode == 'zero' else L // 2 - 1
    NE = N + (1 if odd else 0)
    assert mode == 'zero' or NE == 2 * M
    n = np.arange(NE)
    out = np.zeros(lo.shape[:-1] + (NE,), dt)
    for m in range(L):
        b = n + off - m
        ok = b % 2 == 0
        if mode == 'zero':
            K = b // 2
            ok &= (K >= 0) & (K < M)
        else:
            K = (b % NE) // 2
        idx = np.nonzero(ok)[0]
        out[..., idx] = out[..., idx] + lo[..., K[idx]] * g_lo[m]
        out[..., idx] = out[..., idx] + hi[..., K[idx]] * g_hi[m]
    if odd:
        out[..., N - 1] = out[..., N - 1] + out[..., N]
        out = out[..., :N]
    return np.moveaxis(out, -1, axis)


# ------------------------------------------------------------------------------------------------------------------ the four entry points
def band_of(bits):
    """bits over the transformed axes, slowest first -> index on the band axis"""
    if len(bits) == 3:
        return bits[0] * 4 + bits[1] * 2 + bits[2]
    if len(bits) == 2:
        return bits[1] * 2 + bits[0]
    return bits[0]


def _analysis_nd(x, f_lo, f_hi, mode, nd, odd_rule):
    cur = {(): x}
    for a in range(nd):
        nxt = {}
        for key, v in cur.items():
            nxt[key + (0,)], nxt[key + (1,)] = analysis_1axis(v, f_lo, f_hi, mode, a - nd, odd_rule)
        cur = nxt
    first = cur[(0,) * nd]
    out = np.empty((x.shape[0], 2 ** nd) + first.shape[1:], x.dtype)
    for key, v in cur.items():
        out[:, band_of(key)] = v
    return out


def _synthesis_nd(coef, g_lo, g_hi, mode, nd, sig, odd_rule):
    cur = {key: coef[:, band_of(key)] for key in itertools.product((0, 1), repeat=nd)}
    for a in reversed(range(nd)):
        odd = bool(mode == 'per' and odd_rule and sig[a] & 1)
        cur = {key: synthesis_1axis(cur[key + (0,)], cur[key + (1,)], g_lo, g_hi, mode, sig[a], a - nd, odd)
               for key in itertools.product((0, 1), repeat=a)}
    return cur[()]


def transform(entry, src, taps, mode, nd, sig, dtype=np.float64):
    """entry of ENTRIES; src [n_img, *sig] (analysis-shaped) or [n_img, 2^nd, *coef] (synthesis-shaped); taps = (dec_lo, dec_hi, rec_lo,
    rec_hi), for the kernels' gates the fp32 arrays of real_bank / random_bank; sig = the signal extents of the transformed axes."""
    dl, dh, rl, rh = (np.asarray(t).astype(dtype) for t in taps)
    src = np.asarray(src).astype(dtype)
    if entry == 'fwd':
        return _analysis_nd(src, dl, dh, mode, nd, True)
    if entry == 'inv_adjoint':
        return _analysis_nd(src, rl[::-1], rh[::-1], mode, nd, False)
    if entry == 'inv':
        return _synthesis_nd(src, rl, rh, mode, nd, sig, False)
    if entry == 'fwd_adjoint':
        return _synthesis_nd(src, dl[::-1], dh[::-1], mode, nd, sig, True)
    raise ValueError(entry)


def reference(entry, src, taps, mode, nd, sig):
    """(ref, S_e), both fp64"""
    ref = transform(entry, src, taps, mode, nd, sig)
    scale = transform(entry, np.abs(np.asarray(src, np.float64)), [np.abs(np.asarray(t)) for t in taps], mode, nd, sig)
    return ref, scale


def ratio(got, ref, scale):
    """max over the elements of |got - ref| / (2^-24 S_e); inf where S_e = 0 and got != 0, or got is not finite"""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref)
    if not np.isfinite(got).all():
        return float('inf')
    if ((scale == 0) & (got != 0)).any():
        return float('inf')
    nz = scale > 0
    return float((err[nz] / (U * scale[nz])).max()) if nz.any() else 0.0


# ------------------------------------------------------------------------------------------------------------------ layouts
def coef_strides(nd, cdims, pad=(0, 0)):
    """(cs_img, cs_band, cs0, cs1) of a coefficient tensor whose rows are pad[1] floats longer and whose frames pad[0] floats longer than dense"""
    c3 = [1] * (3 - nd) + list(cdims)
    cs1 = c3[2] + pad[1]
    cs0 = c3[1] * cs1 + pad[0]
    cs_band = c3[0] * cs0
    return (2 ** nd * cs_band, cs_band, cs0, cs1)


def coef_offsets(n_img, nd, cdims, cs):
    """flat offset of every coefficient, shape [n_img, 2^nd, *cdims]"""
    c3 = [1] * (3 - nd) + list(cdims)
    i, b, k0, k1, k2 = np.meshgrid(np.arange(n_img), np.arange(2 ** nd), np.arange(c3[0]), np.arange(c3[1]), np.arange(c3[2]), indexing='ij')
    off = i * cs[0] + b * cs[1] + k0 * cs[2] + k1 * cs[3] + k2
    return off.reshape((n_img, 2 ** nd) + tuple(cdims))


def packed_offsets(n_img, img_inner, cdims, row_w, cs_outer, cs):
    """wdno_dwt_fwd_packed: flat offset of every written element, shape [n_img, 8, To, Ho, row_w]"""
    i, b, k0, k1, k2 = np.meshgrid(np.arange(n_img), np.arange(8), np.arange(cdims[0]), np.arange(cdims[1]), np.arange(row_w), indexing='ij')
    return (i // img_inner) * cs_outer + (i % img_inner) * cs[0] + b * cs[1] + k0 * cs[2] + k1 * cs[3] + k2


def packed_reference(x, taps, sig, img_inner, row_w, resc):
    """(ref, S_e) of the packed analysis, shape [n_img, 8, To, Ho, row_w]: coefficient / rescaler[inner * 8 + band], 0 / rescaler beyond Wo"""
    ref, scale = reference('fwd', x, taps, 'zero', 3, sig)
    n_img, Wo = ref.shape[0], ref.shape[-1]
    r = np.asarray(resc, np.float32).astype(np.float64).reshape(img_inner, 8)[np.arange(n_img) % img_inner][:, :, None, None, None]
    widen = lambda a: np.concatenate([a, np.zeros(a.shape[:-1] + (row_w - Wo,))], axis=-1)
    return widen(ref / r), widen(scale / np.abs(r))


# ------------------------------------------------------------------------------------------------------------------ filters and inputs
def real_bank(name):
    fb = FILTER_BANKS[name]
    return tuple(np.asarray(fb[k], np.float32) for k in ('dec_lo', 'dec_hi', 'rec_lo', 'rec_hi'))


def random_bank(L):
    """four random fp32 tap vectors, all 4 L values distinct in magnitude: no symmetry and no lo / hi relation, so that a reversed, shifted or
    swapped tap moves every output"""
    rng = np.random.default_rng(1000 + L)
    while True:
        t = rng.uniform(0.1, 1.0, 4 * L).astype(np.float32) * rng.choice(np.asarray([-1.0, 1.0], np.float32), 4 * L)
        if len(set(np.abs(t).tolist())) == 4 * L:
            return tuple(t[i * L:(i + 1) * L] for i in range(4))


def bank_of(case):
    return random_bank(case['L']) if case['bank'] == 'rand' else real_bank(case['bank'])


def flat_taps(taps):
    return [float(v) for t in taps for v in t]


def make_input(shape, nd, L, variant, seed):
    """fp32 array; variant 'gauss', 'wide' (gauss * exp(3 gauss): dynamic range per element) or 'edge' (non-zero only within L samples of each
    end of each transformed axis: nothing but the boundary rules contributes)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape)
    if variant == 'wide':
        x = x * np.exp(3.0 * rng.standard_normal(shape))
    elif variant == 'edge':
        for a in range(-nd, 0):
            n = shape[a]
            keep = (np.arange(n) < L) | (np.arange(n) >= n - L)
            x = x * keep.reshape((n,) + (1,) * (-a - 1))
    else:
        assert variant == 'gauss'
    return x.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ geometry of a case
def geometry(case, entry):
    """(signal extents, coefficient extents) of the transformed axes for one entry point. fwd / fwd_adjoint take the case's own signal size;
    inv / inv_adjoint the natural (even) size that its coefficient extents synthesise."""
    L, mode = case['L'], case['mode']
    cdims = [coef_len(n, L, mode) for n in case['sig']]
    if entry in ('inv', 'inv_adjoint'):
        return [natural_len(m, L, mode) for m in cdims], cdims
    return list(case['sig']), cdims


def desc_args(case, entry):
    """(nd, mode id, L, n_img, in_dims, out_dims, cs) as ops.dwt_plan / ops.dwt_call take them"""
    nd = case['nd']
    sig, cdims = geometry(case, entry)
    cs = coef_strides(nd, cdims, case['pad'])
    return nd, MODE_ID[case['mode']], case['L'], case['n_img'], [1] * (3 - nd) + sig, [1] * (3 - nd) + cdims, cs


def src_shape(case, entry):
    sig, cdims = geometry(case, entry)
    return (case['n_img'], *sig) if entry in ANALYSIS_SHAPED else (case['n_img'], 2 ** case['nd'], *cdims)


def case_seed(case, entry, variant):
    """deterministic across processes (hash() of a str is not)"""
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(case['name'] + entry + variant)) % (2 ** 31)


# ------------------------------------------------------------------------------------------------------------------ the case matrix
ANA = ('analysis', 0)
PER_AXIS = ('per_axis', 0)
ALL3 = ('gauss', 'wide', 'edge')
CASES = []


def _case(name, regime, nd, mode, L, sig, expect, bank='rand', n_img=1, variants=('gauss',), debug=0, pad=(0, 0), blocks=None, geom=None):
    """expect: entry -> (family, variant) that ops.dwt_plan must report; geom: entry -> (nh, tiles_h, tiles_t) it must report, given wherever the
    regime is a tile geometry inside a family; blocks: entry -> block count it must report"""
    CASES.append(dict(name=name, regime=regime, nd=nd, mode=mode, L=L, sig=tuple(sig), expect=expect, bank=bank, n_img=n_img, variants=variants,
                      debug=debug, pad=pad, blocks=blocks or {}, geom=geom or {}))


def _fused(ana, syn):
    return {'fwd': ana, 'inv_adjoint': ana, 'inv': syn, 'fwd_adjoint': syn}


S2_1, S2_2, S2F, S3_4, S3_8, S3F = (('synthesis2', 1), ('synthesis2', 2), ('synthesis_fused', 0), ('synthesis3_stream', 4), ('synthesis3_stream', 8),
                                    ('synthesis_fused', 0))

# --- the regimes the choosers' thresholds define, at the filter the Burgers and smoke pipelines use and at random taps
_case('s2-p1-xcd', '2-D synthesis staged, PMAX 1, NH 8, one tile per image, 8 blocks: xcd remap on', 2, 'per', 10, (12, 40), _fused(ANA, S2_1),
      n_img=8, variants=ALL3, blocks={'inv': 8, 'fwd': 8}, geom={'inv': (8, 1, 1), 'fwd': (8, 1, 1)})
_case('s2-p2-two-tiles', '2-D synthesis staged, PMAX 2 (RW 156), two tiles, short last', 2, 'per', 10, (22, 300), _fused(ANA, S2_2), variants=ALL3,
      blocks={'inv': 2}, geom={'inv': (8, 2, 1), 'fwd': (8, 2, 1)})           # 11 q rows: the second tile has 3
_case('s2-p2-lds-cap', '2-D synthesis staged, PMAX 2 near the LDS cap (64 704 B)', 2, 'per', 10, (10, 330), _fused(ANA, S2_2), variants=ALL3, geom={'inv': (8, 1, 1)})
_case('s2f-520', '2-D synthesis unstaged (RW > 256), NH 4: S1 alone', 2, 'per', 10, (10, 520), {'inv': S2F, 'fwd_adjoint': S2F}, variants=ALL3,
      geom={'inv': (4, 2, 1), 'fwd_adjoint': (4, 2, 1)})
_case('s2f-640', '2-D synthesis unstaged, the widest row that fits', 2, 'per', 10, (10, 640), {'inv': S2F, 'fwd_adjoint': S2F},
      geom={'inv': (4, 2, 1)})
_case('s2f-1280-zero', '2-D synthesis unstaged, L = 2, the widest row that fits', 2, 'zero', 2, (4, 1280), {'inv': S2F, 'fwd_adjoint': S2F}, variants=ALL3,
      geom={'inv': (4, 1, 1)})
_case('s2-width-644', '2-D synthesis per-axis by width (nq_max < 4)', 2, 'per', 10, (10, 644), {'inv': PER_AXIS, 'fwd_adjoint': PER_AXIS}, variants=ALL3)
_case('s2-width-1284-zero', '2-D synthesis per-axis by width, L = 2', 2, 'zero', 2, (4, 1284), {'inv': PER_AXIS, 'fwd_adjoint': PER_AXIS})
_case('a2-nh8-512', '2-D analysis NH 8 at its widest row (FW 512)', 2, 'per', 10, (10, 512), {'fwd': ANA, 'inv_adjoint': ANA}, variants=ALL3,
      geom={'fwd': (8, 1, 1), 'inv_adjoint': (8, 1, 1)})
_case('a2-nh4-516', '2-D analysis NH 4 at its narrowest row', 2, 'per', 10, (10, 516), {'fwd': ANA, 'inv_adjoint': ANA},
      geom={'fwd': (4, 2, 1), 'inv_adjoint': (4, 2, 1)})
_case('a2-nh4-1024', '2-D analysis NH 4 at its widest row (FW 1024)', 2, 'per', 10, (10, 1024), {'fwd': ANA, 'inv_adjoint': ANA}, variants=ALL3,
      geom={'fwd': (4, 2, 1), 'inv_adjoint': (4, 2, 1)})
_case('a2-width-1028', '2-D analysis per-axis by width', 2, 'per', 10, (10, 1028), {'fwd': PER_AXIS, 'inv_adjoint': PER_AXIS}, variants=ALL3)
_case('a2-nh4-508-zero', '2-D analysis, zero mode, FW = 2 Wo + L - 2 = 516: NH 4', 2, 'zero', 6, (10, 508), {'fwd': ANA}, geom={'fwd': (4, 2, 1)})
_case('a2-width-1022-zero', '2-D analysis, zero mode, per-axis by width (FW 1030)', 2, 'zero', 6, (10, 1022), {'fwd': PER_AXIS})
_case('s3-w4-ragged', '3-D stream WMAX 4, ragged T and H tiles (NH 7, 2 x 3 tiles)', 3, 'per', 10, (18, 26, 24), _fused(ANA, S3_4), variants=ALL3,
      geom={'inv': (7, 2, 3), 'fwd_adjoint': (7, 2, 3), 'fwd': (7, 2, 3)})       # 13 rows in tiles of 7, 9 frames in tiles of 4 / 3
_case('s3-w4-zero', '3-D stream WMAX 4, zero mode, three H tiles', 3, 'zero', 4, (6, 70, 20), _fused(ANA, S3_4), variants=ALL3,
      geom={'inv': (12, 3, 1), 'fwd': (12, 3, 2)})
_case('s3-w8', '3-D stream WMAX 8 (n_w 1120)', 3, 'per', 10, (10, 12, 80), _fused(ANA, S3_8), variants=ALL3,
      geom={'inv': (3, 2, 2), 'fwd': (1, 6, 2)})                                # the analysis: NH 1, six H tiles
_case('s3f-natural-260', '3-D all-frames kernel without the debug switch: the stream kernel refuses NW > 256, the fused takes FW <= 320', 3, 'per', 2,
      (2, 2, 260), {'inv': S3F, 'fwd_adjoint': S3F}, variants=ALL3, geom={'inv': (1, 1, 1)})
_case('s3f-natural-258-zero', '3-D all-frames kernel without the debug switch, zero mode', 3, 'zero', 2, (2, 2, 258), {'inv': S3F, 'fwd_adjoint': S3F})
_case('s3-width-322', '3-D synthesis per-axis by width, L = 2', 3, 'per', 2, (2, 2, 322), {'inv': PER_AXIS, 'fwd_adjoint': PER_AXIS}, variants=ALL3)
_case('s3-width-208', '3-D synthesis per-axis by width, L = 10', 3, 'per', 10, (10, 10, 208), {'inv': PER_AXIS, 'fwd_adjoint': PER_AXIS})
_case('a3-two-tiles', '3-D analysis: two H tiles of NH 11, To = 7 in tiles of 3 (To % 3 != 0), odd sizes', 3, 'zero', 6, (9, 40, 13), {'fwd': ANA}, variants=ALL3,
      geom={'fwd': (11, 2, 3)})
_case('a3-one-tile', '3-D analysis: one H tile (NH 12 = Ho), To % 3 != 0, odd sizes', 3, 'zero', 6, (9, 20, 13), {'fwd': ANA}, variants=ALL3,
      geom={'fwd': (12, 1, 3)})
_case('a3-330-zero', '3-D analysis at its widest row, L = 2', 3, 'zero', 2, (4, 4, 330), {'fwd': ANA}, geom={'fwd': (1, 2, 1)})
_case('a3-width-344-zero', '3-D analysis per-axis by width, L = 2', 3, 'zero', 2, (4, 4, 344), {'fwd': PER_AXIS}, variants=ALL3)
_case('a3-width-120', '3-D analysis per-axis by width, L = 10', 3, 'per', 10, (10, 10, 120), {'fwd': PER_AXIS, 'inv_adjoint': PER_AXIS})
_case('odd-adjoint-2d', 'periodization fwd_adjoint with an odd length: per-axis by rule, fold-back of position N', 2, 'per', 10, (81, 120),
      {'fwd': ANA, 'fwd_adjoint': PER_AXIS}, variants=ALL3, geom={'fwd': (8, 6, 1)})
_case('odd-adjoint-3d', 'periodization fwd_adjoint with odd lengths, 3-D', 3, 'per', 6, (7, 9, 12), {'fwd': ANA, 'fwd_adjoint': PER_AXIS}, variants=ALL3)

# --- every (L, mode) of every fused kernel at random taps; blocks % 8 == 0 where n_img = 8
for _L, _mode in itertools.product(FUSED_L, ('per', 'zero')):
    _t = f'{_mode}-L{_L}'
    _case(f'sweep2-small-{_t}', '2-D analysis / staged synthesis PMAX 1', 2, _mode, _L, (12, 40), _fused(ANA, S2_1), n_img=3)
    _case(f'sweep2-300-{_t}', '2-D staged synthesis PMAX 2', 2, _mode, _L, (max(6, _L), 300), {'inv': S2_2, 'fwd_adjoint': S2_2, 'fwd': ANA})
    _case(f'sweep2-520-{_t}', '2-D unstaged synthesis', 2, _mode, _L, (max(6, _L), 520), {'inv': S2F, 'fwd_adjoint': S2F, 'fwd': ANA})
    _case(f'sweep3-small-{_t}', '3-D analysis / stream synthesis WMAX 4', 3, _mode, _L, (10, 12, 14), _fused(ANA, S3_4), n_img=2)
    _case(f'sweep3-allframes-{_t}', '3-D all-frames synthesis (debug 45: for L > 2 no shape reaches it otherwise)', 3, _mode, _L, (10, 12, 14),
          _fused(ANA, S3F), n_img=2, debug=DBG_DWT3_SYNTH_LDS)
for _L, _sig in ((6, (6, 6, 176)), (8, (8, 8, 112)), (10, (10, 10, 80))):
    for _mode in ('per', 'zero'):
        _case(f'sweep3-w8-{_mode}-L{_L}', '3-D stream synthesis WMAX 8', 3, _mode, _L, _sig, {'inv': S3_8, 'fwd_adjoint': S3_8})
# blocks % 8 == 0 for the families the cases above leave at other counts
_case('xcd-s2f', '2-D unstaged synthesis, 8 blocks', 2, 'per', 4, (16, 520), {'inv': S2F}, blocks={'inv': 8}, n_img=4)
_case('xcd-s3', '3-D stream and analysis, blocks % 8 == 0', 3, 'per', 6, (8, 12, 14), _fused(ANA, S3_4), n_img=8)
_case('xcd-s3f', '3-D all-frames synthesis, blocks % 8 == 0', 3, 'zero', 4, (8, 12, 14), {'inv': S3F}, n_img=8, debug=DBG_DWT3_SYNTH_LDS)

# --- the smallest legal periodization sizes: wrap_period at its limit (N + odd = L on every transformed axis)
for _L, _nd, _d in itertools.product(FUSED_L, (2, 3), (0, 1)):
    _case(f'per-min-nd{_nd}-L{_L}-N{_L - _d}', 'smallest legal periodization size, N = L' + (' - 1' if _d else ''), _nd, 'per', _L, (_L - _d,) * _nd,
          {'fwd': ANA, 'inv': S2_1 if _nd == 2 else S3_4}, n_img=2, variants=ALL3)

# --- long filters: per-axis kernels only
for _L, _nd, _mode in itertools.product((12, 14, 16), (1, 2, 3), ('per', 'zero')):
    _case(f'long-nd{_nd}-{_mode}-L{_L}', 'filters longer than 10 taps: per-axis', _nd, _mode, _L, ((17,), (16, 19), (16, 17, 20))[_nd - 1],
          {e: PER_AXIS for e in ENTRIES}, n_img=2, variants=ALL3 if (_L, _nd) == (16, 3) else ('gauss',))

# --- 1-D: per-axis, odd and even lengths
for _mode, _L, _n in (('per', 10, 120), ('per', 10, 81), ('per', 2, 7), ('zero', 6, 32), ('zero', 6, 33), ('zero', 8, 21), ('per', 4, 300), ('zero', 2, 513)):
    _case(f'1d-{_mode}-L{_L}-N{_n}', '1-D: per-axis', 1, _mode, _L, (_n,), {e: PER_AXIS for e in ENTRIES}, n_img=3, variants=ALL3 if _n in (81, 33) else ('gauss',))

# --- the real banks (half of them symmetric: the random banks above are what catches a reversed or swapped tap)
for _name, _fb in FILTER_BANKS.items():
    _Lb = len(_fb['dec_lo'])
    _case(f'bank2-{_name}', 'real bank, 2-D periodization', 2, 'per', _Lb, (max(_Lb, 9), 22), {}, bank=_name, n_img=2)
    _case(f'bank3-{_name}', 'real bank, 3-D zero', 3, 'zero', _Lb, (5, 8, 11), {}, bank=_name, n_img=2)

# --- padded (strided) coefficient tensor: cs1 > Wo, cs0 > Ho cs1; the padding keeps its sentinel where the call writes coefficients
_case('padded-2d', 'padded coefficient tensor, 2-D', 2, 'per', 10, (14, 36), _fused(ANA, S2_1), n_img=2, pad=(5, 3), variants=ALL3)
_case('padded-3d', 'padded coefficient tensor, 3-D', 3, 'zero', 6, (8, 10, 12), _fused(ANA, S3_4), n_img=2, pad=(7, 2), variants=ALL3)
_case('padded-3d-allframes', 'padded coefficient tensor, 3-D all-frames synthesis', 3, 'zero', 6, (8, 10, 12), {'inv': S3F, 'fwd_adjoint': S3F}, n_img=2,
      pad=(7, 2), debug=DBG_DWT3_SYNTH_LDS, variants=ALL3)
_case('padded-per-axis', 'padded coefficient tensor, per-axis passes', 3, 'per', 12, (12, 13, 14), {e: PER_AXIS for e in ENTRIES}, n_img=2, pad=(4, 1), variants=ALL3)

BY_NAME = {c['name']: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# --- the packed analysis (wdno_dwt_fwd_packed): 3-D zero, every L; img_inner > 1, row_w > Wo and % 4 == 0, a distinct rescaler per (inner, band),
# rows longer than row_w (their tail keeps its sentinel)
PACKED_CASES = [dict(name=f'packed-L{_L}', L=_L, sig=(6, 9, 10), n_img=6 if _L != 6 else 16, img_inner=2, extra_w=4, tail=4, bank='rand', mode='zero', nd=3)
                for _L in FUSED_L]
PACKED_BY_NAME = {c['name']: c for c in PACKED_CASES}


def packed_layout(c):
    """(cdims, row_w, cs_outer, cs, total floats) of a packed case: state [outer][To][inner * 8 + band][Ho][row_w + tail]"""
    cdims = [coef_len(n, c['L'], 'zero') for n in c['sig']]
    row_w = (cdims[2] + 3) // 4 * 4 + c['extra_w']
    cs1 = row_w + c['tail']
    cs_band = cdims[1] * cs1
    cs_img = 8 * cs_band
    cs0 = c['img_inner'] * cs_img
    cs_outer = cdims[0] * cs0
    return cdims, row_w, cs_outer, (cs_img, cs_band, cs0, cs1), (c['n_img'] // c['img_inner']) * cs_outer


def packed_rescaler(c):
    return (0.5 + np.arange(c['img_inner'] * 8) * 0.173).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ plans and coverage
def plans_of(ops, case):
    """entry -> ops.dwt_plan under the case's debug mode"""
    with ops._lib.debug_mode(case['debug']):
        return {e: ops.dwt_plan(e, *desc_args(case, e)) for e in ENTRIES}


def check_plan(case, entry, p):
    """the case reaches the regime it exists for: return code, LDS within 64 KB, kernel, tile geometry, block count"""
    assert p['rc'] == 0, (entry, p)
    assert p['lds_bytes'] <= 65536, (entry, p)
    if entry in case['expect']:
        assert (p['family'], p['variant']) == case['expect'][entry], (entry, p)
    if entry in case['geom']:
        assert (p['nh'], p['tiles_h'], p['tiles_t']) == case['geom'][entry], (entry, p)
    if entry in case['blocks']:
        assert p['blocks'] == case['blocks'][entry], (entry, p)
    if p['family'] == 'per_axis':
        assert (p['nh'], p['tiles_h'], p['tiles_t'], p['blocks'], p['lds_bytes']) == (0, 0, 0, 0, 0), p
    else:
        assert p['blocks'] == case['n_img'] * p['tiles_t'] * p['tiles_h'] and p['nh'] >= 1, p


def packed_plan(ops, c):
    cdims, row_w, cs_outer, cs, total = packed_layout(c)
    return ops.dwt_plan('fwd_packed', 3, 1, c['L'], c['n_img'], list(c['sig']), cdims, cs)


def coverage_key(plan, L, mode, nd):
    """what one plan adds to the coverage of the matrix"""
    return (plan['family'], plan['variant'], L, mode, nd, plan['blocks'] % 8 == 0)


def check_coverage(ops):
    """every instantiation the choosers can launch is reached by some case, the unreachable ones by none, the 3-D all-frames kernel also
    outside its debug switch, and every fused family with a block count that is a multiple of 8 (xcd_tile renumbers the tiles) and with one
    that is not. Returns a line that says what was reached."""
    seen = {}
    for c in CASES:
        for p in plans_of(ops, c).values():
            k = coverage_key(p, c['L'], c['mode'], c['nd'])
            seen.setdefault(k[:5], set()).add(k[5])
    for c in PACKED_CASES:
        k = coverage_key(packed_plan(ops, c), c['L'], 'zero', 3)
        seen.setdefault(k[:5], set()).add(k[5])
    req = required()
    assert len(req) == 81                                           # 87 instantiations: these, the four unreachable ones, the two per-axis kernels
    missing = sorted(k for k, classes in req.items() if k not in seen or not classes <= seen[k])
    assert not missing, missing
    assert not [k for k in UNREACHABLE if k in seen]
    assert any(k[0] == 'per_axis' for k in seen)
    assert [c['name'] for c in CASES if c['nd'] == 3 and not c['debug'] and c['expect'].get('inv') == ('synthesis_fused', 0)]
    for fam in FAMILIES_BOTH_CLASSES:
        classes = set().union(*(v for k, v in seen.items() if k[0] == fam))
        assert classes == {True, False}, (fam, classes)
    return ('reached: ' + ', '.join(f'{fam} {sum(1 for k in seen if k[0] == fam)}' for fam in ('per_axis',) + FAMILIES_BOTH_CLASSES)
            + f'; not reachable by any shape: {len(UNREACHABLE)}')


# No shape launches these instantiations (the coverage test asserts that the matrix does not either):
#   * dwt_synthesis3_stream_kernel<L = 2 | 4, .., WMAX = 8>: WMAX 8 needs n_w = 4 (NH + E) QW > 1024 W-pass items, and the register budget gives
#     NH <= 512 / (2 NW) = 128 / QW rows, hence NH QW <= 128: n_w <= 512 for L = 2 (E = 0); for L = 4 (E = 1) n_w <= 512 + 4 QW needs QW > 128,
#     where NH would be 0 and the stream kernel refuses.
#   * dwt_synthesis_fused_kernel<3, L > 2, ..> outside debug mode 45: the stream kernel takes every row of NW <= 256 floats it has LDS for, and
#     the all-frames kernel's own budget (40 KB / (2 (4 + E) FW 4 B) rows >= 4 + 2 E) ends at FW = 170, 106, 73, 53 for L = 4, 6, 8, 10, all
#     of which the stream kernel takes. For L = 2 it takes 256 < FW <= 320.
# tests/test_host_dwt_kernels_ref.py::test_unreachable_instantiations sweeps the plan query over coefficient extents to re-check both after a retune.
UNREACHABLE = [('synthesis3_stream', 8, L, mode, 3) for L in (2, 4) for mode in ('per', 'zero')]


def required():
    """(family, variant, L, mode, nd) -> the block-count classes that must occur for that member (none beyond "at least one": the classes are
    asked per family, FAMILIES_BOTH_CLASSES)"""
    req = {}
    for L, mode in itertools.product(FUSED_L, ('per', 'zero')):
        req[('analysis', 0, L, mode, 2)] = set()
        req[('analysis', 0, L, mode, 3)] = set()
        for pmax in (1, 2):
            req[('synthesis2', pmax, L, mode, 2)] = set()
        for wmax in (4, 8):
            req[('synthesis3_stream', wmax, L, mode, 3)] = set()
        for nd in (2, 3):
            req[('synthesis_fused', 0, L, mode, nd)] = set()
    for L in FUSED_L:
        req[('analysis_packed', 0, L, 'zero', 3)] = set()
    for key in UNREACHABLE:
        del req[key]
    return req


# per fused family (over all L, modes and variants): both block-count classes
FAMILIES_BOTH_CLASSES = ('analysis', 'analysis_packed', 'synthesis2', 'synthesis_fused', 'synthesis3_stream')
