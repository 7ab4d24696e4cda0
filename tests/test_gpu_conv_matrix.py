"""Convolution kernels (wdno_amd/csrc/conv*.hip, linear_rows.hip, through wdno_amd.ops) against tests/conv_ref.py, element by element, on
a case matrix that visits every launch regime the library's own plan queries name: exact fp32, the register-staged, chunked-DMA and
tap-resident forward / data-gradient kernels in every tile shape, the split runs, the stem, and the register-staged, chunked, window and
stem weight gradients with their split reductions.

Two gates. Families int1 and int2 are built so that every partial sum is exactly representable: the kernels must return the reference's
bits (torch.equal), and the amax records must be max|.| exactly. Families gauss and range are held to |got - ref| <= K 2^-24 scale with
the scales and K of tests/conv_ref.py (K comes from the fp32 transcription there, not from these kernels). Every case first asserts,
from the library's plan query on the device, that it still reaches the regime it exists for, and afterwards that the launches that
happened are the ones those plans were asked about."""
import math

import pytest
import torch

from tests import conv_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
IDS = [c.name for c in R.CASES]


@pytest.fixture(scope='module')
def ops():
    from wdno_amd import ops as o
    o._lib_()          # fails loudly if libwdno_hip.so is missing
    return o


def _to_cl(v, cpad):
    """[N, C, *sp] fp32 CPU -> [N, *sp, cpad] on the device, zero padded."""
    cl = v.permute(0, *range(2, v.dim()), 1)
    out = torch.zeros(*cl.shape[:-1], cpad, dtype=torch.float32)
    out[..., :v.shape[1]] = cl
    return out.to(DEV).contiguous()


def _from_cl(v, c):
    return v.detach().cpu().permute(0, v.dim() - 1, *range(1, v.dim() - 1))[:, :c].contiguous()


def _run(ops, case, family, flat=None):
    """One forward + backward through ops.conv_cl. Returns ({name: CPU tensor in the reference layout}, extras). A 2-D case is fed as a
    5-D tensor with D = 1 (the geometry ops.conv_cl makes of a 4-D input, so the same launches): the amax records then stay on the
    results, which a 4-D input's reshaped results do not carry. extras['routes']: which of ops.split_f16_colsum / colsum / conv_fwd_raw ran."""
    t = R.inputs(case, family)
    n, c, k, sp, ks, st, pd, osp = R.dims(case)
    cp, kp = ops.pad4(c), ops.pad4(k)
    nd = len(case.ws) - 2
    up = (lambda v: v.unsqueeze(1)) if nd == 2 else (lambda v: v)          # CL [N, H, W, C] -> [N, 1, H, W, C]
    x = up(_to_cl(t['x'], cp)).requires_grad_(True)
    w = t['w'].reshape(k, c, *ks).to(DEV).requires_grad_(True)
    b = t['bias'].to(DEV).requires_grad_(True) if case.bias else None
    res = up(_to_cl(t['res'], kp)).requires_grad_(True) if case.residual else None
    dy = up(_to_cl(t['dy'], kp))
    if case.zbox is not None:
        ops.set_zero_box(x, case.zbox)
    if flat is not None:                          # the trainer's flat gradient buffer: the weight gradient is written there by a deferred reduction
        w._wdno_flat_grad, w._wdno_flat_busy = flat, False
    seen = []
    x.register_hook(seen.append)
    ex = {'routes': []}
    spied = {name: getattr(ops, name) for name in ('split_f16_colsum', 'colsum', 'conv_fwd_raw')}

    def spy(name):
        def call(*a, **kw):
            ex['routes'].append(name)
            return spied[name](*a, **kw)
        return call
    for name in spied:
        setattr(ops, name, spy(name))
    try:
        if case.skip:
            y, xs = ops.conv_cl_skip(x, w, b, stride=st, padding=pd)
            ex['rec_y'] = ops._known_amax(y)
            torch.autograd.backward([y, xs], [dy, up(_to_cl(t['skip'], cp))])
        else:
            y = ops.conv_cl(x, w, b, stride=st, padding=pd, residual=res)
            ex['rec_y'] = ops._known_amax(y)
            y.backward(dy)
    finally:
        for name, fn in spied.items():
            setattr(ops, name, fn)
    down = (lambda v: v.squeeze(2)) if nd == 2 else (lambda v: v)          # [N, C, 1, H, W] -> [N, C, H, W]
    out = {'y': down(_from_cl(y, k)), 'dx': down(_from_cl(seen[0], c)), 'dw': w.grad.detach().cpu().reshape(case.ws)}
    assert float(y.detach()[..., k:].abs().max() if kp > k else 0.0) == 0.0 and float(seen[0][..., c:].abs().max() if cp > c else 0.0) == 0.0
    ex['rec_dx'] = ops._known_amax(seen[0])
    ex['wgrad'] = w.grad
    if case.bias:
        out['db'] = b.grad.detach().cpu()
    if case.residual:
        out['dres'] = down(_from_cl(res.grad, k))
    return out, ex


def _record_max(rec):
    return float(rec.reshape(-1, 16)[:, 0].max())          # one slot per 64-byte line (WDNO_AMAX_STRIDE floats)


def _check_records(case, ex, values):
    """The amax records the split kernels leave on y and dx are max|.| exactly, on every case whose pass runs on a split kernel."""
    for name, rec, plan in (('y', ex['rec_y'], case.plan[0]), ('dx', ex['rec_dx'], case.plan[1])):
        if plan is not None:
            assert rec is not None, (case.name, 'no amax record on', name)
        if rec is not None:
            assert _record_max(rec) == float(values[name].abs().max()), (case.name, 'amax record of', name)


def _check_routes(ops, case, ex):
    """The bias gradient comes from the pass that splits dy (ops.split_f16_colsum) wherever dy is split, from ops.colsum otherwise -- also
    inside split_f16_colsum, for plane widths that are no power-of-two number of 8-channel groups; the exact-fp32 forward is conv_fwd_raw."""
    routes = ex['routes']
    g8 = ops.pad8(ops.pad4(case.ws[0])) // 8
    fused = g8 <= 256 and g8 & (g8 - 1) == 0
    if case.bias:
        assert ('split_f16_colsum' in routes) == (case.plan[2] is not None), (case.name, routes)
        assert ('colsum' in routes) == (case.plan[2] is None or not fused), (case.name, routes)
    assert ('conv_fwd_raw' in routes) == (case.plan[0] is None), (case.name, routes)


def _check_planes(ops, case, family):
    """ops.split_f16 and ops.split_weight return the emulation's planes and scales bit for bit: a disagreement about a scale shows up here
    and not as a kernel failure."""
    t = R.inputs(case, family)
    n, c, k, sp, ks, st, pd, osp = R.dims(case)
    cp, kp = ops.pad4(c), ops.pad4(k)
    c8 = ops.pad8(cp)
    for key, cpad in (('x', cp), ('dy', kp)):
        v = _to_cl(t[key], cpad)
        hi, lo, s = ops.split_f16(v.reshape(-1, cpad))
        eh, el, es = R.planes(t[key])
        assert float(s) == es, (case.name, family, key, float(s), es)
        for got, want in ((hi, eh), (lo, el)):
            wcl = _to_cl(want.float(), ops.pad8(cpad)).reshape(-1, ops.pad8(cpad))
            assert torch.equal(got.float(), wcl), (case.name, family, key)
    w = t['w'].to(DEV)
    hi, lo, s = ops.split_weight(w, 'f', c8, kp)
    eh, el, es = R.planes(t['w'])
    assert float(s) == es, (case.name, family, 'w', float(s), es)
    for got, want in ((hi, eh), (lo, el)):
        w5 = want.float().reshape(k, c, *ks)
        packed = torch.zeros(ks[0], ks[1], kp, ks[2], c8)
        packed[:, :, :k, :, :c] = w5.permute(2, 3, 0, 4, 1)
        assert torch.equal(got.float().cpu().reshape(packed.shape), packed), (case.name, family, 'w')


def _check_launches(ops, case, log):
    """The launches that happened are the launches the plans were asked about (tests/conv_ref.py::launches)."""
    want = R.launches(ops, case)
    assert len(log) == len(want), (case.name, log, want)
    for e, (_, kind, g, extra) in zip(log, want):
        assert (e[0], e[1], e[2]) == (kind, ops._geom_fields(g), extra[0]), (case.name, e, kind, ops._geom_fields(g))
        if kind == 'fwd':           # the residual flag, and the plan under the workspace the launch really lent is the plan that was asserted
            assert e[3] == extra[1], (case.name, e)
            assert R.fwd_plan_str(ops.conv_fwd_plan(g, e[2], False, e[4])) == R.plan_of(ops, kind, g, extra), (case.name, e)
        else:
            assert e[3] == extra[1], (case.name, e)


# int2 is a statement about planes: the exact-fp32 kernels multiply the values themselves and run int1 only
EXACT = [(c, f) for c in R.CASES for f in ('int1', 'int2') if f == 'int1' or c.plan[0] is not None]


@pytest.mark.parametrize('case,family', EXACT, ids=[f'{c.name}-{f}' for c, f in EXACT])
def test_exact(ops, case, family):
    """The kernels return the reference's bits: y, dx, dw, db and the residual gradient, and the amax records; two runs, equal bits."""
    want = R.expected(case, family)
    with ops._lib.debug_mode(case.mode):
        assert R.plans(ops, case) == case.plan, (case.name, R.plans(ops, case), case.plan)
        if case.plan[0] is not None:
            _check_planes(ops, case, family)
        ops.LAUNCH_LOG = log = []
        try:
            got, ex = _run(ops, case, family)
        finally:
            ops.LAUNCH_LOG = None
        _check_launches(ops, case, log)
        again, _ = _run(ops, case, family)
    bad = [R.wrong_elements(got[name], want[name], name, case) for name in want]
    assert not any(bad), (case.name, family, [b for b in bad if b])
    assert got.keys() == want.keys()
    for name in got:
        assert torch.equal(got[name], again[name]), (case.name, family, name, 'two runs differ')
    _check_records(case, ex, want)
    _check_routes(ops, case, ex)


GATED = [(c, f) for c in R.CASES for f in R.families(c) if f in ('gauss', 'range')]


@pytest.mark.parametrize('case,family', GATED, ids=[f'{c.name}-{f}' for c, f in GATED])
def test_elementwise(ops, case, family):
    """|got - ref| <= K 2^-24 scale (+ the sub-normal flush of the lo planes) for every element of y, dx, dw and db."""
    ref, scale, flush = R.expected(case, family)
    with ops._lib.debug_mode(case.mode):
        assert R.plans(ops, case) == case.plan
        got, ex = _run(ops, case, family)
        again, _ = _run(ops, case, family)
    bad = []
    for name in ('y', 'dx', 'dw', 'db'):
        if name not in got:
            continue
        assert torch.isfinite(got[name]).all(), (case.name, family, name)
        r, k = R.ratio(got[name], ref[name], scale[name], flush[name]), R.k_of(case, name)
        print(f'GATE {case.name} {family} {name}: {r:.2f} / {k}  [{case.plan[{"y": 0, "dx": 1, "dw": 2, "db": 2}[name]]}]')
        if not r <= k:
            bad.append((name, round(r, 2), k))
    assert not bad, (case.name, family, bad)
    if case.residual:
        assert torch.equal(got['dres'], R.inputs(case, family)['dy'])
    for name in got:
        assert torch.equal(got[name], again[name]), (case.name, family, name, 'two runs differ')
    _check_records(case, ex, got)


DEFERRED = ['wgrad_mode70', 'wgrad_pair_odd', 'tap_64x64', 'stem_192', 'reg_64x64_ksplit2']


def test_deferred_weight_gradient_reduction(ops):
    """Inside ops.flat_wgrad_scope() the split reductions of several convolutions run as ONE wdno_wgrad_reduce_multi launch when the backward
    has returned, the tiled and the plain form side by side: the gradients land in the flat buffer and equal the immediate ones bit for bit,
    which equal the reference's bits."""
    cases = [R.BY_NAME[n] for n in DEFERRED]
    forms = {('tiled' in c.plan[2]) for c in cases}
    assert forms == {True, False}
    flats = [torch.full((math.prod(c.ws),), float('nan'), device=DEV) for c in cases]
    imm = []
    for c in cases:
        with ops._lib.debug_mode(c.mode):
            imm.append(_run(ops, c, 'int2')[0]['dw'])
    with ops.flat_wgrad_scope():
        assert ops._WGRAD_PENDING == []
        grads = []
        for c, flat in zip(cases, flats):
            with ops._lib.debug_mode(c.mode):
                grads.append(_run(ops, c, 'int2', flat=flat)[1]['wgrad'])
        assert len(ops._WGRAD_PENDING) == len(cases)          # nothing reduced yet
    for c, flat, g, want in zip(cases, flats, grads, imm):
        assert g.data_ptr() == flat.data_ptr(), c.name
        assert torch.equal(flat.reshape(c.ws).cpu(), want), c.name
        assert torch.equal(want, R.expected(c, 'int2')['dw']), c.name


@pytest.mark.parametrize('rows', [1, 8, 64, 65])
def test_linear_rows_exact(ops, rows):
    """nn.Linear on a handful of rows (linear_rows.hip; from 65 rows on the convolution path): int1 inputs, the reference's bits."""
    from tests.helpers import _hash_values
    cin, cout = 96, 40
    ints = lambda shape, seed: torch.floor(torch.from_numpy(_hash_values(math.prod(shape), seed).reshape(shape)) * 9.0 + 4.5) - 4.0
    x, w, b, dy = ints((rows, cin), 1 + rows), ints((cout, cin), 2), ints((cout,), 3), ints((rows, cout), 4 + rows)
    want = {'y': x @ w.t() + b, 'dx': dy @ w, 'dw': dy.t() @ x, 'db': dy.sum(0)}
    runs = []
    raw, calls = ops.conv_fwd_raw, []
    ops.conv_fwd_raw = lambda *a, **kw: (calls.append(1), raw(*a, **kw))[1]
    try:
        for _ in range(2):
            xd, wd, bd = (v.float().to(DEV).requires_grad_(True) for v in (x, w, b))
            y = ops.conv_cl(xd, wd, bd)
            y.backward(dy.float().to(DEV))
            runs.append({'y': y.detach().cpu(), 'dx': xd.grad.cpu(), 'dw': wd.grad.cpu(), 'db': bd.grad.cpu()})
    finally:
        ops.conv_fwd_raw = raw
    # 65 rows: the exact-fp32 convolution kernel, forward and data gradient of both runs; up to 64 rows: linear_rows.hip, never that kernel
    assert len(calls) == (4 if rows > ops.LINEAR_ROWS_MAX else 0), (rows, calls)
    assert ops.LINEAR_ROWS_MAX == 64
    for name, v in want.items():
        assert torch.equal(runs[0][name].double(), v), (rows, name)
        assert torch.equal(runs[0][name], runs[1][name]), (rows, name)


@pytest.mark.parametrize('case,plan', R.BF16_CASES, ids=[c.name for c, _ in R.BF16_CASES])
def test_single_plane_bf16(ops, case, plan):
    """ops._math('bf16'): one bf16 plane per operand, one product. int1 is exact in bf16, so the reference's bits; gauss within K16 2^-9
    scale (db, a sum of the fp32 dy, within its fp32 gate); two runs, equal bits."""
    with ops._math('bf16'), ops._lib.debug_mode(case.mode):
        assert R.plans(ops, case, lowp=True) == plan
        ops.LAUNCH_LOG = log = []
        try:
            got, _ = _run(ops, case, 'int1')
        finally:
            ops.LAUNCH_LOG = None
        assert [(e[0], e[1], e[2]) for e in log] == [(kind, ops._geom_fields(g), True) for _, kind, g, _ in R.launches(ops, case, lowp=True)]
        again, _ = _run(ops, case, 'int1')
        gauss, _ = _run(ops, case, 'gauss')
    want = R.expected(case, 'int1')
    bad = [R.wrong_elements(got[name], want[name], name, case) for name in want]
    assert not any(bad), (case.name, [b for b in bad if b])
    for name in got:
        assert torch.equal(got[name], again[name]), (case.name, name, 'two runs differ')
    ref, scale, flush = R.expected(case, 'gauss')
    out = []
    for name in ('y', 'dx', 'dw', 'db'):
        if name not in gauss:
            continue
        k = R.K16.get(name)
        r = R.ratio(gauss[name], ref[name], scale[name], None, R.U16) if k else R.ratio(gauss[name], ref[name], scale[name])
        k = k or R.k_of(case, name)
        print(f'GATE16 {case.name} gauss {name}: {r:.2f} / {k}  [{plan[{"y": 0, "dx": 1, "dw": 2, "db": 2}[name]]}]')
        if not r <= k:
            out.append((name, round(r, 2), k))
    assert not out, (case.name, out)


@pytest.mark.parametrize('family', ['int1', 'int2'])
def test_conv_transpose_exact(ops, family):
    """ops.conv_transpose_cl (four parity-class launches of the split kernels, the strided convolution as its data gradient, the weight
    gradient with x and dy in exchanged roles): the reference's bits, and two runs agree."""
    t = R.convt_inputs(family)
    want = {k: v.float() for k, v in R.convt_reference(t, True).items()}
    cin, cout = t['w'].shape[:2]
    runs = []
    for _ in range(2):
        x = _to_cl(t['x'], cin).requires_grad_(True)
        w, b = t['w'].to(DEV).requires_grad_(True), t['bias'].to(DEV).requires_grad_(True)
        ops.LAUNCH_LOG = log = []
        try:
            y = ops.conv_transpose_cl(x, w, b)
            y.backward(_to_cl(t['dy'], cout))
        finally:
            ops.LAUNCH_LOG = None
        assert [e[0] for e in log] == ['fwd'] * 5 + ['wgrad'], log          # the split kernels ran: four parity classes, dx, dw
        runs.append({'y': _from_cl(y, cout), 'dx': _from_cl(x.grad, cin), 'dw': w.grad.cpu(), 'db': b.grad.cpu()})
    for name in want:
        assert torch.equal(runs[0][name], want[name]), (family, name, int((runs[0][name] != want[name]).sum()), 'elements differ')
        assert torch.equal(runs[0][name], runs[1][name]), (family, name)


def test_linear_multi_exact(ops):
    """ops.linear_multi: several nn.Linear layers on the same rows in one launch, forward and backward (linear_rows.hip): int1 inputs,
    the reference's bits for every output, dx (the sum over the layers) and every weight / bias gradient."""
    from tests.helpers import _hash_values
    ints = lambda shape, seed: torch.floor(torch.from_numpy(_hash_values(math.prod(shape), seed).reshape(shape)) * 9.0 + 4.5) - 4.0
    rows, cin, outs = 8, 64, (32, 64, 24)
    x = ints((rows, cin), 21)
    ws, bs, dys = [ints((k, cin), 30 + i) for i, k in enumerate(outs)], [ints((k,), 40 + i) for i, k in enumerate(outs)], [ints((rows, k), 50 + i) for i, k in enumerate(outs)]
    layers = []
    for w, b in zip(ws, bs):
        lin = torch.nn.Linear(cin, w.shape[0]).to(DEV)
        with torch.no_grad():
            lin.weight.copy_(w.float())
            lin.bias.copy_(b.float())
        layers.append(lin)
    xd = x.float().to(DEV).requires_grad_(True)
    ys = ops.linear_multi(xd, layers)
    assert ys is not None and len(ys) == len(outs)
    torch.autograd.backward(ys, [dy.float().to(DEV) for dy in dys])
    for y, w, b in zip(ys, ws, bs):
        assert torch.equal(y.detach().cpu().double(), x @ w.t() + b)
    assert torch.equal(xd.grad.cpu().double(), sum(dy @ w for dy, w in zip(dys, ws)))
    for lin, dy in zip(layers, dys):
        assert torch.equal(lin.weight.grad.cpu().double(), dy.t() @ x) and torch.equal(lin.bias.grad.cpu().double(), dy.sum(0))


def test_patch2_data_gradient_on_the_fp32_kernels(ops):
    """ops.PATCH_DGRAD_H3 off: the data gradient of the folded 2 x 2 / stride-2 patch convolution as four exact-fp32 launches -- the same
    bits as the four split-kernel launches on int1 inputs, which are the reference's."""
    case = R.BY_NAME['patch2']
    want = R.expected(case, 'int1')
    ops.PATCH_DGRAD_H3 = False
    try:
        ops.LAUNCH_LOG = log = []
        got, _ = _run(ops, case, 'int1')
    finally:
        ops.PATCH_DGRAD_H3, ops.LAUNCH_LOG = True, None
    assert [e[0] for e in log] == ['fwd', 'wgrad'], log            # no split-kernel launch for the data gradient
    for name in want:
        assert torch.equal(got[name], want[name]), name


def _out16_cases():
    return [(c, pl) for c, pl in R.BF16_CASES if not c.residual and (c.ws[0] + 3) // 4 * 4 % 8 == 0]


@pytest.mark.parametrize('case,plan', _out16_cases(), ids=[c.name for c, _ in _out16_cases()])
def test_single_plane_bf16_output_store(ops, case, plan):
    """The out16 store of the single-plane forward (wdno_conv_fwd_bf16_ex, y_bf16 = 1): y as bf16 storage is the fp32 result rounded to
    nearest even -- on int1 inputs the reference's integers rounded once to bf16, bit for bit."""
    t = R.inputs(case, 'int1')
    n, c, k, sp, ks, st, pd, osp = R.dims(case)
    cp, kp = ops.pad4(c), ops.pad4(k)
    want = torch.zeros(n, *osp, kp)
    want[..., :k] = R.expected(case, 'int1')['y'].reshape(n, k, *osp).permute(0, 2, 3, 4, 1)
    x = _to_cl(t['x'].reshape(n, c, *sp), cp)
    w = t['w'].reshape(k, c, *ks).to(DEV)
    with ops._math('bf16'), ops._lib.debug_mode(case.mode), torch.no_grad():
        assert R.plans(ops, case, lowp=True)[0] == plan[0]
        planes = ops.split_f16(x.reshape(-1, cp))
        assert planes[1] is None
        bias_p = ops._pad_vec(t['bias'].to(DEV) if case.bias else None, kp)
        runs = [ops.conv_fwd_h3(planes, (n, *sp), w, ops.pack_fwd, 'f', bias_p, None, ks, st, pd, kp, out16=True) for _ in range(2)]
    assert runs[0].dtype == torch.bfloat16 and tuple(runs[0].shape) == tuple(want.shape)
    assert float(want.abs().max()) > 256.0                     # beyond the integers bf16 holds exactly: the rounding is exercised
    assert torch.equal(runs[0].cpu(), want.to(torch.bfloat16)), (case.name, int((runs[0].cpu() != want.to(torch.bfloat16)).sum()), 'elements differ')
    assert torch.equal(runs[0], runs[1])


@pytest.mark.parametrize('family', ['int1', 'int2'])
def test_split_refused_for_lack_of_workspace(ops, family):
    """wdno_conv_fwd_f16x3_ws on a geometry that wants the four-run split, with no workspace and with too small a one: the unsplit
    64 x 64 tap-resident kernel runs (the plan says so) and returns the reference's bits; with the workspace, the split does."""
    import ctypes as C
    from wdno_amd import _lib
    case = R.BY_NAME['split4_mode56']                          # the geometry of split4_residual with a bias and no residual
    t = R.inputs(case, family)
    n, c, k, sp, ks, st, pd, osp = R.dims(case)
    (_, _, g, _), = [l for l in R.launches(ops, case) if l[0] == 'y']
    lib = ops._lib_()
    need = int(lib.wdno_conv_fwd_split_ws_bytes(C.byref(g)))
    assert need == 4 * n * sp[0] * sp[1] * sp[2] * k * 4
    x = _to_cl(t['x'], c)
    xh, xl, sx = ops.split_f16(x.reshape(-1, c))
    wh, wl, sw = ops.split_weight(t['w'].to(DEV), 'f', c, k)
    bias = t['bias'].to(DEV)
    want = R.expected(case, family)['y']
    for ws_bytes, plan in ((0, 'h3t:64x64 t64 g64'), (need // 2, 'h3t:64x64 t64 g64'), (need, 'h3t:128x128/4 t16 g64')):
        assert R.fwd_plan_str(ops.conv_fwd_plan(g, False, False, ws_bytes)) == plan
        y = torch.full((n, *osp, k), float('nan'), device=DEV)
        ws = torch.empty(max(ws_bytes, 4) // 4, device=DEV) if ws_bytes else None
        _lib.check(lib.wdno_conv_fwd_f16x3_ws(ops._p(xh), ops._p(xl), ops._p(sx), ops._p(wh), ops._p(wl), ops._p(sw), ops._p(bias), None, ops._p(y),
                                              None, C.byref(g), ops._p(ws), ws_bytes, ops._stream()), 'conv_fwd_f16x3_ws')
        bad = R.wrong_elements(_from_cl(y, k), want, 'y', case)
        assert not bad, (family, ws_bytes, bad)


ONE_SPLIT = R._c('stem_one_split', (1, 42, 2, 16, 16), (16, 42, 3, 3, 7), padding=(1, 1, 3))


@pytest.mark.parametrize('family', ['int1', 'int2'])
def test_stem_weight_gradient_one_split_straight_to_the_destination(ops, family):
    """The stem weight gradient with splits == 1 writes the packed destination itself, no reduction (wdno_conv_wgrad_f16x3 through
    ops.conv_wgrad_h3 without a parameter layout). ops.conv_cl cannot reach it -- from 1024 pixels on the plan has at least two splits
    (tests/test_host_conv_ref.py) and below it runs the exact-fp32 kernels -- so the planes are made here: the reference's bits."""
    case = ONE_SPLIT
    t = R.inputs(case, family)
    n, c, k, sp, ks, st, pd, osp = R.dims(case)
    cp, kp = ops.pad4(c), ops.pad4(k)
    g = ops._geom((n, *sp), 48, ops.pad8(kp), ks, st, pd, osp)
    assert R.wgrad_plan_str(ops.conv_wgrad_plan(g, False, k, c)).startswith('h3s:64x352 s1 ')
    xp = ops.split_f16(_to_cl(t['x'], cp).reshape(-1, cp), c8=48)
    gp = ops.split_f16(_to_cl(t['dy'], kp).reshape(-1, kp))
    runs = [ops.conv_wgrad_h3(xp, (n, *sp), gp, osp, ks, st, pd) for _ in range(2)]
    assert tuple(runs[0].shape) == (ks[0], ks[1], ops.pad8(kp), ks[2], 48)
    got = runs[0][:, :, :k, :, :c].permute(2, 4, 0, 1, 3).contiguous().cpu()
    bad = R.wrong_elements(got, R.expected(case, family)['dw'], 'dw', case)
    assert not bad, (family, bad)
    assert float(runs[0][:, :, k:].abs().max() if ops.pad8(kp) > k else 0.0) == 0.0 and float(runs[0][..., c:].abs().max()) == 0.0
    assert torch.equal(runs[0], runs[1])
