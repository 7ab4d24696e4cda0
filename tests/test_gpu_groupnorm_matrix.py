"""GroupNorm kernels (wdno_amd/csrc/norm.hip, through wdno_amd.ops) against the fp64 reference of tests/groupnorm_ref.py, element by
element, on a case matrix that visits every launch regime of the kernels: chunk counts 1 .. 256 (odd, unrolled by eight, uneven pieces,
a short last chunk), 1 .. 32 finalize slices (several groups each, idle slices, a short last slice), narrow / wide groups on both sides
of cg = 64, one to 256 lanes per row, S = 1, N = 1 and N > 64, and the planes forms where eight channels of a thread span several groups.

The gate is |got - ref| <= K 2^-24 scale with the scales and the K of tests/groupnorm_ref.py (K comes from the fp32 transcription there,
not from these kernels). Every case first asserts, from the library's own answers, that it still reaches the regime it exists for."""
import ctypes as C
import math

import pytest
import torch

from tests import groupnorm_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PLANES = [cv for cv in R.MATRIX if R.planes_ok(cv[0][2])]


@pytest.fixture(scope='module')
def ops():
    from wdno_amd import ops as o
    o._lib_()          # fails loudly if libwdno_hip.so is missing
    return o


@pytest.mark.parametrize('case,nchunk,rows', [c[:3] for c in R.CASES], ids=[R.case_id((c[0], 'std')) for c in R.CASES])
def test_case_reaches_its_regime(ops, case, nchunk, rows):
    """nchunk (from the workspace size: ws = 16 N nchunk C + 16 N C + 16 N G + 64 bytes) and the rows of column-sum partials of the planes
    backward (N x blocks per sample) are what the case was chosen for; a retune of the heuristics has to revisit the matrix.
    And the tail the planes forms carve out of their workspace -- from the next 64-byte boundary behind the plain workspace: forward the
    per-chunk maxima (N x nchunk x 2 floats), backward N x CAP rows of C fp64 column-sum partials and the maxima behind them -- fits the size
    the library asks for."""
    lib = ops._lib_()
    n, s, c, g = case
    ws = int(lib.wdno_groupnorm_ws_bytes(n, s, c, g))
    num = ws - 16 * n * c - 16 * n * g - 64
    assert num % (16 * n * c) == 0 and num // (16 * n * c) == nchunk, (num / (16 * n * c), nchunk)
    off, prow = C.c_size_t(0), C.c_int(0)
    assert lib.wdno_groupnorm_bwd_planes_tail(n, s, c, g, C.byref(off), C.byref(prow)) == 0
    if rows is not None:
        assert prow.value == rows, (prow.value, rows)
    assert R.planes_ok(c) == (rows is not None)
    CAP = 128                                             # blocks per sample of the planes backward at the most
    align64 = lambda b: (b + 63) // 64 * 64
    assert off.value == align64(ws), (off.value, ws)
    assert off.value + n * CAP * c * 8 + n * nchunk * 2 * 4 <= int(lib.wdno_groupnorm_bwd_planes_ws_bytes(n, s, c, g))
    assert prow.value <= n * CAP, (prow.value, n * CAP)
    assert align64(ws) + n * nchunk * 2 * 4 <= int(lib.wdno_groupnorm_fwd_planes_ws_bytes(n, s, c, g))


def _dev(t, grad=False):
    return t.to(DEV).requires_grad_(grad)


def _run(ops, case, variant, act, use_ss, mode):
    """One forward + backward. mode 'fp32': groupnorm_act; 'add': groupnorm_act_add; 'planes': groupnorm_act whose input is marked as
    taking its gradient as fp16 planes (what conv_cl(..., grad_planes=True) states about its output). Returns ({name: tensor}, extras)."""
    t = R.inputs(case, variant)
    x, gam, bet = _dev(t['x'], True), _dev(t['gamma'], True), _dev(t['beta'], True)
    ss = _dev(t['ss'], True) if use_ss else None
    dy = _dev(t['dy'])
    seen = []
    x.register_hook(seen.append)
    out, ex = {}, {}
    if mode == 'planes':
        x._wdno_grad_planes = True
    if mode == 'add':
        res = _dev(t['res'], True)
        y = ops.groupnorm_act_add(x, gam, bet, case[3], res, ss, act=act)
        out['y_add'] = y.detach().clone()
    else:
        y = ops.groupnorm_act(x, gam, bet, case[3], ss, act=act)
        out['y'] = y.detach().clone()
    if mode != 'planes':
        ex['rec_y'] = ops._known_amax(y)
    y.backward(dy)
    dx = seen[0]
    if mode == 'planes':
        (hi, lo, scale), cs = dx._wdno_planes_only[0], dx._wdno_planes_only[1]
        ex['hi'], ex['lo'], ex['scale'] = hi.clone(), lo.clone(), scale.clone()
        out['colsum'] = cs.clone()
    else:
        out['dx'] = dx.detach().clone()
        ex['rec_dx'] = ops._known_amax(dx)
    if mode == 'add':
        ex['dres'], ex['dy'] = res.grad, dy
    out['dgamma'], out['dbeta'] = gam.grad.clone(), bet.grad.clone()
    if use_ss:
        out['dss'] = ss.grad.clone()
    return out, ex


def _gate(label, got, ref, extra=None):
    bad = []
    for name, v in got.items():
        assert torch.isfinite(v).all(), (label, name)
        r = R.ratio(v, ref[0][name], ref[1][name], None if extra is None else extra.get(name))
        k = R.K[R.KIND[name]]
        print(f'{label} {name}: {r:.2f} / {k}')
        if not r <= k:
            bad.append((name, round(r, 2), k))
    assert not bad, (label, bad)


def _same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), k


def _record_is_exact(rec, t):
    assert rec is not None
    assert float(rec.reshape(-1, 16)[:, 0].max()) == float(t.abs().max())       # one slot per 64-byte line (WDNO_AMAX_STRIDE floats)


@pytest.mark.parametrize('cv', R.MATRIX, ids=R.case_id)
def test_fp32_route(ops, cv):
    """(a) y, dx, dgamma, dbeta, dss element-wise; (c) the amax records on y and dx are max|.| exactly; (f) two calls, equal bits."""
    case, variant = cv
    for act, use_ss in R.configs(case):
        ref = R.reference_of(case, variant, act, use_ss)
        got, ex = _run(ops, case, variant, act, use_ss, 'fp32')
        _gate(f'{R.case_id(cv)} act={act} ss={use_ss}', got, ref)
        _record_is_exact(ex['rec_y'], got['y'])
        _record_is_exact(ex['rec_dx'], got['dx'])
        again, _ = _run(ops, case, variant, act, use_ss, 'fp32')
        _same_bits(got, again)


@pytest.mark.parametrize('cv', R.MATRIX, ids=R.case_id)
def test_act_add(ops, cv):
    """(b) act(GroupNorm(x)) + residual: the sum is gated, the residual's gradient is dy bit for bit, the other gradients as in (a)."""
    case, variant = cv
    for act, use_ss in R.configs(case):
        ref = R.reference_of(case, variant, act, use_ss)
        got, ex = _run(ops, case, variant, act, use_ss, 'add')
        _gate(f'{R.case_id(cv)} add act={act} ss={use_ss}', got, ref)
        assert torch.equal(ex['dres'], ex['dy'])
        if R.planes_ok(case[2]):                      # the fused apply pass (other channel counts: norm, then an add)
            _record_is_exact(ex['rec_y'], got['y_add'])
        again, _ = _run(ops, case, variant, act, use_ss, 'add')
        _same_bits(got, again)


def _planes_checks(label, ex, ref_v, ref_scale, kind, amax, bound):
    hi, lo, sc = ex['hi'], ex['lo'], float(ex['scale'])
    assert torch.isfinite(hi).all() and torch.isfinite(lo).all(), label
    assert sc > 0 and math.frexp(sc)[0] == 0.5, (label, sc)                     # a power of two
    assert sc * amax < 2.0 ** 15, (label, sc, amax)                             # no value overflows the hi plane
    assert sc >= 2.0 ** 13 / bound * (1 - 2.0 ** -20), (label, sc, bound)       # and the analytic bound is no looser than it may be
    v = ((hi.double() + lo.double()) / sc).cpu().reshape(ref_v.shape)
    r = R.ratio(v, ref_v, ref_scale, R.rep_allowance(ref_v, sc))
    print(f'{label} planes of {kind}: {r:.2f} / {R.K[kind]}, scale {sc}, scale * amax {sc * amax:.1f}, scale * bound {sc * bound:.1f}')
    assert r <= R.K[kind], (label, r)


@pytest.mark.parametrize('cv', PLANES, ids=R.case_id)
def test_forward_planes(ops, cv):
    """(d) out_planes=True: (hi + lo) / scale against the fp64 y, and the scale against the bound it is derived from."""
    case, variant = cv
    t = R.inputs(case, variant)
    x, gam, bet = _dev(t['x']), _dev(t['gamma']), _dev(t['beta'])
    for act, use_ss in R.configs(case):
        ref = R.reference_of(case, variant, act, use_ss)
        runs = []
        for _ in range(2):
            with torch.no_grad():
                yp = ops.groupnorm_act(x, gam, bet, case[3], _dev(t['ss']) if use_ss else None, act=act, out_planes=True)
            hi, lo, scale = yp._wdno_planes[0]
            runs.append({'hi': hi.clone(), 'lo': lo.clone(), 'scale': scale.clone()})
        _planes_checks(f'{R.case_id(cv)} act={act} ss={use_ss}', runs[0], ref[0]['y'], ref[1]['y'], 'y', ref[2]['amax_y'], ref[2]['bound_y'])
        _same_bits(runs[0], runs[1])


@pytest.mark.parametrize('cv', PLANES, ids=R.case_id)
def test_backward_planes(ops, cv):
    """(e) dx as planes with the bound of gn_bwd_finalize_kernel, its column sums, and the parameter gradients of the same launch sequence
    (N = 1: the per-sample pieces themselves; N > 1: their sum over the samples)."""
    case, variant = cv
    for act, use_ss in R.configs(case):
        ref = R.reference_of(case, variant, act, use_ss)
        label = f'{R.case_id(cv)} act={act} ss={use_ss}'
        got, ex = _run(ops, case, variant, act, use_ss, 'planes')
        _planes_checks(label, ex, ref[0]['dx'], ref[1]['dx'], 'dx', ref[2]['amax_dx'], ref[2]['bound_dx'])
        _gate(label + ' planes', got, ref)
        again, ex2 = _run(ops, case, variant, act, use_ss, 'planes')
        _same_bits(got, again)
        _same_bits(ex, ex2)
