"""Anchors tests/dwt_kernels_ref.py -- the fp64 reference, the error scale and the gate the wavelet kernels are held to in
tests/test_gpu_dwt_matrix.py -- without a GPU: against PyWavelets (tests/golden/dwt_pywt.npz) at the precision the fixture is stored in, against
oracle/dwt_ref.py, by the adjoint identity <A x, y> = <x, A^T y> for both adjoint pairs, and by perfect reconstruction for the real banks. For
every case of the matrix the fp32 transcription (every product and add rounded, no fma) stays within K: the bound is shown to hold for a correct
implementation before any kernel is held to it. The plan query needs no device either: every case reaches the regime it names, no plan asks for
more than 64 KB of LDS, and the matrix as a whole reaches every instantiation the choosers can launch."""
import itertools

import numpy as np
import pytest

from oracle import dwt_ref as O
from tests import dwt_kernels_ref as R
from tests.helpers import load_npz
from wdno_amd.filters import FILTER_BANKS

G = load_npz('dwt_pywt.npz')
TOL = 1e-12
MODE_OF = {'periodization': 'per', 'zero': 'zero'}


def bank64(name):
    fb = FILTER_BANKS[name]
    return tuple(np.asarray(fb[k], np.float64) for k in ('dec_lo', 'dec_hi', 'rec_lo', 'rec_hi'))


def close(a, b, tol=TOL):
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max())


def flat(x, nd):
    return x.reshape((-1,) + x.shape[-nd:])


def fwd64(x, wave, mode, nd):
    """[..., *sig] -> [n_img, 2^nd, *coef] with fp64 taps"""
    return R.transform('fwd', flat(x, nd), bank64(wave), mode, nd, list(x.shape[-nd:]))


def inv64(packed, wave, mode, nd):
    L = len(FILTER_BANKS[wave]['dec_lo'])
    return R.transform('inv', packed, bank64(wave), mode, nd, [R.natural_len(m, L, mode) for m in packed.shape[-nd:]])


def crop_like(ll, ref_shape, nd):
    """an approximation one sample longer than the next detail band loses its last sample before the synthesis (pywt.waverec*)"""
    sl = [slice(None)] * ll.ndim
    for a in range(-nd, 0):
        if ll.shape[a] == ref_shape[a] + 1:
            sl[a] = slice(0, -1)
    return ll[tuple(sl)]


# ------------------------------------------------------------------------------------------------------------------ PyWavelets fixtures
def _groups(prefix):
    return sorted({k[len(prefix):].rsplit('_', 1)[0] for k in G.files if k.startswith(prefix)})


def test_every_fixture_group_is_visited():
    """the tests below cover every key of the fixture file"""
    heads = {k.split('_')[0] for k in G.files}
    assert heads == {'dwt2per', 'idwt2per', 'dwt1', 'idwt1', 'dwt2zero', 'dwt3', 'idwt3', 'wavedec1', 'waverec1', 'wavedec2', 'waverec2', 'wavedec3',
                     'waverec3'}, heads


@pytest.mark.parametrize('tag', _groups('dwt2per_'))
def test_pywt_dwt2_periodization(tag):
    w = str(G[f'dwt2per_{tag}_wave'])
    got = fwd64(G[f'dwt2per_{tag}_x'], w, 'per', 2)
    want = flat(np.concatenate([G[f'dwt2per_{tag}_yl'][:, :, None], G[f'dwt2per_{tag}_yh']], axis=2), 3)
    assert close(got, want)
    packed = flat(np.concatenate([G[f'idwt2per_{tag}_yl'][:, :, None], G[f'idwt2per_{tag}_yh']], axis=2), 3)
    assert close(inv64(packed, w, 'per', 2), flat(G[f'idwt2per_{tag}_x'], 2))


@pytest.mark.parametrize('tag', _groups('dwt2zero_'))
def test_pywt_dwt2_zero(tag):
    got = fwd64(G[f'dwt2zero_{tag}_x'], str(G[f'dwt2zero_{tag}_wave']), 'zero', 2)
    assert close(got, flat(np.concatenate([G[f'dwt2zero_{tag}_yl'][:, :, None], G[f'dwt2zero_{tag}_yh']], axis=2), 3))


@pytest.mark.parametrize('tag', _groups('dwt1_'))
def test_pywt_dwt1(tag):
    w, m = str(G[f'dwt1_{tag}_wave']), MODE_OF[str(G[f'dwt1_{tag}_mode'])]
    got = fwd64(G[f'dwt1_{tag}_x'], w, m, 1)
    assert close(got, flat(np.stack([G[f'dwt1_{tag}_lo'], G[f'dwt1_{tag}_hi']], axis=2), 2))
    packed = flat(np.stack([G[f'idwt1_{tag}_lo'], G[f'idwt1_{tag}_hi']], axis=2), 2)
    assert close(inv64(packed, w, m, 1), flat(G[f'idwt1_{tag}_x'], 1))


@pytest.mark.parametrize('tag', _groups('dwt3_'))
def test_pywt_dwt3_zero(tag):
    w = str(G[f'dwt3_{tag}_wave'])
    assert close(fwd64(G[f'dwt3_{tag}_x'], w, 'zero', 3), G[f'dwt3_{tag}_coef'])
    assert close(inv64(G[f'idwt3_{tag}_coef'], w, 'zero', 3), G[f'idwt3_{tag}_x'])


@pytest.mark.parametrize('tag', _groups('wavedec1_'))
def test_pywt_multilevel_1d(tag):
    w, m, J = str(G[f'wavedec1_{tag}_wave']), MODE_OF[str(G[f'wavedec1_{tag}_mode'])], int(G[f'wavedec1_{tag}_J'])
    lo, his = flat(G[f'wavedec1_{tag}_x'], 1), []
    for lvl in range(J):
        c = fwd64(lo, w, m, 1)
        lo = c[:, 0]
        his.append(c[:, 1])
        assert close(his[-1], flat(G[f'wavedec1_{tag}_hi{lvl}'], 1))
    assert close(lo, flat(G[f'wavedec1_{tag}_lo'], 1))
    for hi in his[::-1]:
        lo = inv64(np.stack([crop_like(lo, hi.shape, 1), hi], axis=1), w, m, 1)
    assert close(lo, flat(G[f'waverec1_{tag}_x'], 1))


@pytest.mark.parametrize('tag', _groups('wavedec2_'))
def test_pywt_multilevel_2d(tag):
    w, J = str(G[f'wavedec2_{tag}_wave']), int(G[f'wavedec2_{tag}_J'])
    ll, yh = flat(G[f'wavedec2_{tag}_x'], 2), []
    for lvl in range(J):
        c = fwd64(ll, w, 'per', 2)
        ll = c[:, 0]
        yh.append(c[:, 1:])
        assert close(yh[-1], flat(G[f'wavedec2_{tag}_yh{lvl}'], 3))
    assert close(ll, flat(G[f'wavedec2_{tag}_yl'], 2))
    ll = flat(G[f'waverec2_{tag}_yl'], 2)
    for lvl in reversed(range(J)):
        h = flat(G[f'waverec2_{tag}_yh{lvl}'], 3)
        ll = inv64(np.concatenate([crop_like(ll, h.shape, 2)[:, None], h], axis=1), w, 'per', 2)
    assert close(ll, flat(G[f'waverec2_{tag}_x'], 2))


@pytest.mark.parametrize('tag', _groups('wavedec3_'))
def test_pywt_multilevel_3d(tag):
    w, J = str(G[f'wavedec3_{tag}_wave']), int(G[f'wavedec3_{tag}_J'])
    lll, det = G[f'wavedec3_{tag}_x'], []
    for _ in range(J):
        c = fwd64(lll, w, 'zero', 3)
        lll = c[:, 0]
        det.append(c[:, 1:])
    assert close(lll, G[f'wavedec3_{tag}_lll'])
    for lvl, d in enumerate(det[::-1]):                       # the fixture lists the coarsest level first
        assert close(d, G[f'wavedec3_{tag}_d{lvl}'])
    for d in det[::-1]:
        lll = inv64(np.concatenate([crop_like(lll, d.shape, 3)[:, None], d], axis=1), w, 'zero', 3)
    assert close(lll, G[f'waverec3_{tag}_x'])


# ------------------------------------------------------------------------------------------------------------------ oracle/dwt_ref.py
SHAPES = {1: [(3, 24), (2, 33)], 2: [(2, 16, 24), (2, 19, 21)], 3: [(2, 12, 10, 16), (1, 11, 13, 9)]}


@pytest.mark.parametrize('wave', sorted(FILTER_BANKS))
@pytest.mark.parametrize('mode', ['periodization', 'zero'])
def test_oracle_agrees_in_fp64_and_in_fp32_to_rounding(wave, mode):
    """oracle/dwt_ref.py computes in the dtype of its input: in float64 it is the reference to 1e-12; in float32 (another order of the same sums) it
    lies within the gate K 2^-24 S_e of the fp64 reference with fp32 taps, as any correct fp32 implementation must"""
    m = MODE_OF[mode]
    L = len(FILTER_BANKS[wave]['dec_lo'])
    rng = np.random.default_rng(L)
    for nd, shapes in SHAPES.items():
        for shape in shapes:
            if m == 'per' and min(s + (s & 1) for s in shape[1:]) < L:
                continue
            x = rng.standard_normal(shape)

            def oracle(xx):
                xx = xx[:, None]
                if nd == 1:
                    return np.stack(O.dwt1d(xx, wave, mode), axis=2)[:, 0]
                if nd == 2:
                    yl, yh = O.dwt2(xx, wave, mode)
                    return np.concatenate([yl[:, :, None], yh], axis=2)[:, 0]
                return O.smoke_coef_to_tensor(*O.dwt3(xx[:, 0], wave, mode))
            c64 = oracle(x)
            assert close(fwd64(x, wave, m, nd), c64)
            x32 = x.astype(np.float32)
            ref, scale = R.reference('fwd', x32, R.real_bank(wave), m, nd, list(shape[1:]))
            got = oracle(x32)                                 # (the oracle rounds its taps to the dtype of its input: the same fp32 taps)
            assert got.dtype == np.float32
            assert R.ratio(got, ref, scale) <= R.gate_k(nd, L), (nd, shape)
            # the inverse, from the fp64 coefficients
            if nd == 1:
                back = O.idwt1d(c64[:, None, 0], c64[:, None, 1], wave, mode)[:, 0]
            elif nd == 2:
                back = O.idwt2(c64[:, None, 0], c64[:, None, 1:], wave, mode)[:, 0]
            else:
                back = O.idwt3(c64[:, 0], {k: c64[:, i + 1] for i, k in enumerate(O.BANDS3[1:])}, wave, mode)
            assert close(inv64(c64, wave, m, nd), back)


# ------------------------------------------------------------------------------------------------------------------ properties of the reference
@pytest.mark.parametrize('nd', [1, 2, 3])
@pytest.mark.parametrize('mode', ['per', 'zero'])
@pytest.mark.parametrize('L', R.ALL_L)
def test_adjoint_identity(nd, mode, L):
    """<A x, y> = <x, A^T y> for (fwd, fwd_adjoint) and (inv, inv_adjoint), random taps, even and odd lengths (the odd periodized fold-back)"""
    taps = R.random_bank(L)
    rng = np.random.default_rng(7 * L + nd)
    for sig in ([L + 4, L + 7, L + 2][:nd], [L + 3, L - 1, L + 1][:nd], [L - 1] * nd):
        if mode == 'zero' and min(sig) < 1:
            continue
        cd = [R.coef_len(n, L, mode) for n in sig]
        x = rng.standard_normal((2, *sig))
        y = rng.standard_normal((2, 2 ** nd, *cd))
        ax = R.transform('fwd', x, taps, mode, nd, sig)
        aty = R.transform('fwd_adjoint', y, taps, mode, nd, sig)
        assert aty.shape == x.shape
        assert abs((ax * y).sum() - (x * aty).sum()) <= TOL * (np.abs(ax) * np.abs(y)).sum()
        nat = [R.natural_len(m, L, mode) for m in cd]
        z = rng.standard_normal((2, *nat))
        by = R.transform('inv', y, taps, mode, nd, nat)
        btz = R.transform('inv_adjoint', z, taps, mode, nd, nat)
        assert by.shape == z.shape and btz.shape == y.shape
        assert abs((by * z).sum() - (y * btz).sum()) <= TOL * (np.abs(by) * np.abs(z)).sum()


def bank_defect(wave):
    """how far the published taps are from a perfect-reconstruction pair, from the two polynomial identities and not from the reference:
    rec_lo(z) dec_lo(z) + rec_hi(z) dec_hi(z) = 2 z^-(L-1) and rec_lo(z) dec_lo(-z) + rec_hi(z) dec_hi(-z) = 0"""
    dl, dh, rl, rh = bank64(wave)
    L = len(dl)
    alt = (-1.0) ** np.arange(L)
    p = np.convolve(rl, dl) + np.convolve(rh, dh)
    p[L - 1] -= 2.0
    q = np.convolve(rl, dl * alt) + np.convolve(rh, dh * alt)
    return max(np.abs(p).max(), np.abs(q).max())


@pytest.mark.parametrize('wave', sorted(FILTER_BANKS))
@pytest.mark.parametrize('mode', ['per', 'zero'])
def test_perfect_reconstruction_of_the_real_banks(wave, mode):
    """inv(fwd(x)) = x up to fp64 rounding plus the bank's own defect: per axis, 2 L - 1 product coefficients off by at most bank_defect, on
    samples below 6 in magnitude (the published sym4 taps are a perfect-reconstruction pair to 2e-12 only; every other bank to 1e-15)"""
    L = len(FILTER_BANKS[wave]['dec_lo'])
    rng = np.random.default_rng(3)
    for nd in (1, 2, 3):
        x = rng.standard_normal((2, *[12, 16, 10][:nd]))
        assert np.abs(x).max() < 6
        assert close(inv64(fwd64(x, wave, mode, nd), wave, mode, nd), x, TOL + nd * (2 * L - 1) * 6 * bank_defect(wave))


def test_bank_defects():
    assert all(bank_defect(w) < 1e-14 for w in FILTER_BANKS if w != 'sym4') and bank_defect('sym4') < 1e-11


def test_random_banks_have_no_symmetry():
    for L in R.ALL_L:
        t = np.concatenate(R.random_bank(L))
        assert t.dtype == np.float32 and len(set(np.abs(t).tolist())) == 4 * L


def test_edge_input_is_zero_away_from_the_ends():
    x = R.make_input((2, 30, 40), 2, 4, 'edge', 1)
    assert np.count_nonzero(x[:, 4:-4, :]) == 0 and np.count_nonzero(x[:, :, 4:-4]) == 0 and np.count_nonzero(x[:, :4, :4]) == 32


# ------------------------------------------------------------------------------------------------------------------ the gate holds on the CPU
@pytest.mark.parametrize('name', list(R.BY_NAME))
def test_fp32_transcription_stays_within_the_gate(name):
    c = R.BY_NAME[name]
    taps = R.bank_of(c)
    K = R.gate_k(c['nd'], c['L'])
    for entry, variant in itertools.product(R.ENTRIES, c['variants']):
        sig, _ = R.geometry(c, entry)
        src = R.make_input(R.src_shape(c, entry), c['nd'], c['L'], variant, R.case_seed(c, entry, variant))
        ref, scale = R.reference(entry, src, taps, c['mode'], c['nd'], sig)
        got = R.transform(entry, src, taps, c['mode'], c['nd'], sig, np.float32)
        assert got.dtype == np.float32
        assert R.ratio(got, ref, scale) <= K, (entry, variant)


@pytest.mark.parametrize('name', list(R.PACKED_BY_NAME))
def test_fp32_transcription_of_the_packed_analysis(name):
    c = R.PACKED_BY_NAME[name]
    taps, resc = R.bank_of(c), R.packed_rescaler(c)
    cdims, row_w, cs_outer, cs, total = R.packed_layout(c)
    assert c['img_inner'] > 1 and row_w > cdims[2] and row_w % 4 == 0 and cs[3] > row_w and len(set(resc.tolist())) == len(resc)
    x = R.make_input((c['n_img'], *c['sig']), 3, c['L'], 'wide', 5)
    ref, scale = R.packed_reference(x, taps, list(c['sig']), c['img_inner'], row_w, resc)
    got = R.transform('fwd', x, taps, 'zero', 3, list(c['sig']), np.float32)
    got = got / resc.reshape(c['img_inner'], 8)[np.arange(c['n_img']) % c['img_inner']][:, :, None, None, None]
    assert got.dtype == np.float32
    got = np.concatenate([got, np.zeros(got.shape[:-1] + (row_w - cdims[2],), np.float32)], axis=-1)
    assert R.ratio(got, ref, scale) <= R.gate_k(3, c['L'], packed=True)
    off = R.packed_offsets(c['n_img'], c['img_inner'], cdims, row_w, cs_outer, cs)
    assert off.max() < total and len(np.unique(off)) == off.size


# ------------------------------------------------------------------------------------------------------------------ plans (no device needed)
@pytest.fixture(scope='module')
def ops():
    from wdno_amd import ops as o
    o._lib_()
    return o


plans_of = R.plans_of


@pytest.mark.parametrize('name', list(R.BY_NAME))
def test_case_reaches_its_regime(ops, name):
    """kernel, variant, tile geometry (nh, tiles_h, tiles_t wherever the regime names them) and block count, from the plan"""
    c = R.BY_NAME[name]
    for e, p in plans_of(ops, c).items():
        R.check_plan(c, e, p)


def test_every_geometry_regime_states_its_geometry():
    """a case whose regime text names rows per tile or a tile count carries the numbers the plan must report"""
    import re
    for c in R.CASES:
        if re.search(r'\bNH \d|\btiles?\b', c['regime']):
            assert c['geom'], c['name']


def test_unstaged_2d_synthesis_asks_for_s1_alone(ops):
    """dwt_synthesis_fused_kernel<2, ..> has no staged rows: per_row (NH + E) bytes. Periodization, L = 10, W = 520: 4 160 x 8 = 33 280 (the
    request used to add the staged rows of dwt_synthesis2_kernel: 67 072, and 82 432 / 81 920 at the two shapes below -- past 64 KB)"""
    p = plans_of(ops, R.BY_NAME['s2f-520'])['inv']
    assert (p['family'], p['nh'], p['lds_bytes']) == ('synthesis_fused', 4, 33280), p
    for name, want in (('s2f-640', 2 * 640 * 4 * 8), ('s2f-1280-zero', 2 * 1280 * 4 * 4)):
        p = plans_of(ops, R.BY_NAME[name])['inv']
        assert p['family'] == 'synthesis_fused' and p['lds_bytes'] == want <= 65536, p


def test_plan_follows_the_debug_modes_and_reports_refusals(ops):
    c = R.BY_NAME['s3-w4-ragged']
    with ops._lib.debug_mode(R.DBG_PER_AXIS_DWT):
        assert {p['family'] for p in plans_of(ops, dict(c, debug=R.DBG_PER_AXIS_DWT)).values()} == {'per_axis'}
    assert plans_of(ops, dict(c, debug=R.DBG_DWT3_SYNTH_LDS))['inv']['family'] == 'synthesis_fused'
    assert plans_of(ops, c)['inv']['family'] == 'synthesis3_stream'
    nd, mode, L, n_img, ind, outd, cs = R.desc_args(c, 'fwd')
    assert ops.dwt_plan('fwd', nd, mode, 5, n_img, ind, outd, cs)['rc'] != 0                  # odd filter length
    bad = ops.dwt_plan('inv', nd, mode, L, n_img, [d + 1 for d in ind], outd, cs)               # not the natural size
    assert bad['rc'] != 0 and bad['family'] is None
    small = ops.dwt_plan('fwd', 2, 0, 10, 1, [1, 6, 40], [1, 3, 20], R.coef_strides(2, [3, 20]))   # periodization shorter than the filter
    assert small['rc'] != 0


_packed_plan = R.packed_plan


def test_packed_plan(ops):
    for c in R.PACKED_CASES:
        p = _packed_plan(ops, c)
        assert p['rc'] == 0 and p['family'] == 'analysis_packed' and p['lds_bytes'] <= 65536, p
    c = R.PACKED_CASES[0]
    cdims, row_w, cs_outer, cs, total = R.packed_layout(c)
    assert ops.dwt_plan('fwd_packed', 3, 0, 10, 2, [10, 10, 10], [5, 5, 5], R.coef_strides(3, [5, 5, 5]))['rc'] != 0       # periodization: not taken
    wide = ops.dwt_plan('fwd_packed', 3, 1, 2, 1, [4, 4, 344], [2, 2, 172], R.coef_strides(3, [2, 2, 172]))                # rows too wide for LDS
    assert wide['rc'] != 0 and wide['family'] is None


def test_coverage(ops):
    """every instantiation the choosers can launch is reached by some case, the unreachable ones by none, and every fused family is launched
    with a block count that is a multiple of 8 and with one that is not (R.check_coverage, shared with the GPU test)"""
    print(R.check_coverage(ops))


def test_unreachable_instantiations(ops):
    """R.UNREACHABLE, re-checked by a sweep of the plan query over 3-D coefficient extents (every row width up to 400, the row counts at which
    the tile choice changes, two frame counts): the stream kernel never reports WMAX 8 for L = 2 and L = 4 and does for L = 6, 8, 10; without
    debug mode 45 the all-frames kernel is reached for L = 2 only"""
    seen = set()
    for L, mode in itertools.product(R.FUSED_L, ('per', 'zero')):
        for cH, cW, cT in itertools.product(list(range(max(1, L // 2), 14)) + [40, 100], range(max(1, L // 2), 400), (max(2, L // 2), 9)):
            cd = [cT, cH, cW]
            sig = [R.natural_len(m, L, mode) for m in cd]
            p = ops.dwt_plan('inv', 3, R.MODE_ID[mode], L, 1, sig, cd, R.coef_strides(3, cd))
            if p['rc'] == 0:
                seen.add((p['family'], p['variant'], L, mode, 3))
    assert not [k for k in R.UNREACHABLE if k in seen]
    assert {k for k in seen if k[0] == 'synthesis3_stream' and k[1] == 8} == {('synthesis3_stream', 8, L, m, 3) for L in (6, 8, 10) for m in ('per', 'zero')}
    assert {k for k in seen if k[0] == 'synthesis_fused'} == {('synthesis_fused', 0, 2, m, 3) for m in ('per', 'zero')}
