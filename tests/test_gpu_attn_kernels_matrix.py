"""The layer-by-layer attention kernels (csrc/attention.hip, csrc/linattn.hip) and the channel LayerNorm (csrc/layernorm.hip) held ELEMENT BY ELEMENT to the fp64
references of tests/attn_kernels_ref.py, |got - ref| <= K 2^-24 scale + flush, on a case matrix that visits every launch regime the plan queries
(ops.attn_plan, ops.linattn_plan, ops.layernorm_plan) can report: every kernel family, one item up to a grid-stride walk with a second pass, the
bias-gradient partial in registers and in LDS, every chunk count edge of the linear attention, every (lanes per row, vectors per lane) pair of the
LayerNorm. K comes from the CPU transcription (tests/test_host_attn_kernels_ref.py), not from the kernels. Every case asserts from the plan that it
reaches the regime it exists for. Also here: exact amax records, bit-reproducibility (dbias included), results that do not depend on which block or
pass handled a unit, untouched rows between strided units, and the refusals: the code the plan reports, nothing written. The kernels are called
through ops.softmax_attention / linear_attention / layernorm_cl(_skip), the way production reaches them; the refusals and the plane-delivering
forms through the library's entry points, whose buffers the test can pre-fill. The plane forms (wdno_attn_fwd_planes / _bwd_planes,
wdno_linattn_fwd_planes / _bwd_planes, wdno_layernorm_fwd_planes): the delivered scale is the one the documented bound implies, the bound holds,
no entry saturates, hi / s + lo / s is held to the fp64 reference with the split's own rounding added to the gate, the single bf16 plane in
units of 2^-9, and the planes are bit for bit the split of what the fp32 form writes."""
import ctypes as C
import math

import pytest
import torch

from tests import attn_kernels_ref as R
from tests.attn_ref import scale_from_amax

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = -7.25


@pytest.fixture(scope='module')
def ops():
    from wdno_amd import ops as o
    o._lib_()
    assert torch.cuda.get_device_properties(0).multi_processor_count == R.CUS, 'the regimes of tests/attn_kernels_ref.py are stated for %d compute units' % R.CUS
    return o


def dev(t, grad=False):
    if t is None:
        return None
    x = t.to(torch.float32).to(DEV).contiguous()
    return x.requires_grad_(True) if grad else x


def _gate(block, got, ref, label):
    out, scale = ref
    rel = {}
    for name, kind in R.KIND[block].items():
        if name in got:
            assert torch.isfinite(got[name]).all(), name
            rel[name] = R.ratio(got[name], out[name], scale[name], torch.full_like(out[name], R.FLUSH)) / R.K[kind]
    print(f'{label}: ratio / K  ' + '  '.join(f'{k} {v:.3f}' for k, v in rel.items()))
    bad = {k: v for k, v in rel.items() if not v <= 1.0}
    assert not bad, (label, bad)
    return rel


def _record_is_exact(ops, t, what):
    rec = ops._known_amax(t)
    assert rec is not None, what
    assert float(rec.max()) == float(t.detach().abs().max()), what


def _subset(plan, want):
    return {k: plan.get(k) for k in want}


# ------------------------------------------------------------------------------------------------------------------ softmax attention
def _attn_plans(ops, c):
    lay = c['lay']
    pf = ops.attn_plan('fwd', c['heads'], *lay[:6], rot=c['rot'], bias=c['bias'])
    pb = ops.attn_plan('bwd', c['heads'], *lay[:6], rot=c['rot'], bias=c['bias'], dbias=c['dbias'])
    return pf, pb


def _attn_run(ops, c, t):
    """one forward (+ backward) through ops.softmax_attention: {out, dqkv, dbias} as device tensors"""
    lay = c['lay']
    qkv = dev(t['qkv'], c['bwd'])
    bias = dev(t['bias'], c['dbias'])
    rot = None if t['cos'] is None else (dev(t['cos']), dev(t['sin']))
    out = ops.softmax_attention(qkv, c['heads'], lay[0], lay[1], lay[2], lay[3], lay[4], lay[5], R.SCALE, bias=bias, rot=rot)
    got = {'out': out.detach()}
    _record_is_exact(ops, out, 'out')
    if c['bwd']:
        seen = {}
        qkv.register_hook(lambda g_: seen.__setitem__('g', g_))
        out.backward(dev(t['dout']))
        got['dqkv'] = qkv.grad
        _record_is_exact(ops, seen['g'], 'dqkv')
        if c['dbias']:
            got['dbias'] = bias.grad
    return got


@pytest.mark.parametrize('name', list(R.A_BY_NAME))
def test_attention_gate(ops, name):
    c, t = R.A_BY_NAME[name], R.a_inputs(name)
    with ops._lib.debug_mode(c['debug']):
        pf, pb = _attn_plans(ops, c)
        assert pf['rc'] == 0 and _subset(pf, c['fwd']) == c['fwd'], pf
        if c['bwd']:
            assert pb['rc'] == 0 and _subset(pb, c['back']) == c['back'], pb
        got = _attn_run(ops, c, t)
        again = _attn_run(ops, c, t)
    _gate('attn', got, R.reference_of_a(name), name)
    for k in got:                                                         # two runs: equal bits, the bias gradient included
        assert torch.equal(got[k], again[k]), k


@pytest.mark.parametrize('name', ['cap+1-24', 'cap+1-2', 'groups-wrap', 'tiledbwd-wrap', 'big-wrap'])
def test_a_unit_does_not_depend_on_the_block_or_pass_that_handled_it(ops, name):
    """the first and the last unit of a walk with a second pass are given the same rows: equal bits out"""
    c, t = R.A_BY_NAME[name], dict(R.a_inputs(name))
    pf, pb = _attn_plans(ops, c)
    assert pb['max_walk'] >= 2
    idx = t['idx']
    t['qkv'], t['dout'] = t['qkv'].clone(), t['dout'].clone()
    t['qkv'][idx[-1]], t['dout'][idx[-1]] = t['qkv'][idx[0]], t['dout'][idx[0]]
    got = _attn_run(ops, c, t)
    first, last = idx[0].to(DEV), idx[-1].to(DEV)
    assert torch.equal(got['out'][first], got['out'][last]) and torch.equal(got['dqkv'][first], got['dqkv'][last])


def _desc(ops, lay, heads):
    return ops.AttnDesc(lay[0], lay[1], lay[2], heads, lay[3], lay[4], lay[5])


def _filled(*shape, dtype=torch.float32):
    return torch.full(shape, SENTINEL, device=DEV, dtype=dtype)


@pytest.mark.parametrize('what,n,tables', [('fwd', 1025, False), ('bwd', 577, False), ('bwd', 129, True), ('bwd', 128, True), ('bwd-dbias', 78, True),
                                           ('bwd-planes', 33, True), ('fwd-planes', 65, True)])
def test_attention_refusals_write_nothing(ops, what, n, tables):
    """Beyond its limits a call returns the code the plan reports -- decided by the host code before any launch -- and leaves its outputs alone."""
    lib, p = ops._lib_(), ops._p
    heads, hd = 4, 128
    lay = R.layout('spatial', 2, 1, n)
    d = _desc(ops, lay, heads)
    rows = lay[6]
    g = torch.Generator().manual_seed(n)
    qkv, dout, fout = dev(torch.randn(rows, 3 * hd, generator=g)), dev(torch.randn(rows, hd, generator=g)), dev(torch.randn(rows, hd, generator=g))
    cos = sin = bias = None
    if tables:
        cos, sin = (dev(x) for x in R.rot_tables(1.0 / (10000 ** (torch.arange(0, 32, 2).double() / 32)), n))
        bias = dev(torch.randn(heads, n, n, generator=g))
    planes, dbias = what.endswith('planes'), what == 'bwd-dbias'
    plan = ops.attn_plan(what[:3], heads, *lay[:6], rot=tables, bias=tables, dbias=dbias, planes=planes)
    assert plan['rc'] == -3 and plan['family'] is None, plan
    outs = [_filled(rows, hd if what.startswith('fwd') else 3 * hd)]
    rec = torch.zeros(ops.AMAX_FLOATS, device=DEV)
    st = ops._stream()
    if what == 'fwd':
        rc = lib.wdno_attn_fwd_amax(p(qkv), p(cos), p(sin), p(bias), p(outs[0]), p(rec), C.byref(d), R.SCALE, st)
    elif what == 'fwd-planes':
        outs += [_filled(rows, hd, dtype=torch.float16), _filled(rows, hd, dtype=torch.float16), _filled(1)]
        rc = lib.wdno_attn_fwd_planes(p(qkv), p(cos), p(sin), p(bias), p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), p(rec), p(rec), C.byref(d), R.SCALE, st)
    elif what == 'bwd-planes':
        outs = [_filled(rows, 3 * hd, dtype=torch.float16), _filled(rows, 3 * hd, dtype=torch.float16), _filled(1)]
        rc = lib.wdno_attn_bwd_planes(p(qkv), p(cos), p(sin), p(bias), p(fout), p(dout), p(outs[0]), p(outs[1]), p(outs[2]), None, p(rec), p(rec),
                                      C.byref(d), R.SCALE, None, 0, st)
    else:
        ws = None
        if dbias:
            outs.append(_filled(heads, n, n))
            ws = _filled(lib.wdno_attn_bwd_ws_bytes(C.byref(d)) // 4 + 4)
            outs.append(ws)
        rc = lib.wdno_attn_bwd_amax(p(qkv), p(cos), p(sin), p(bias), p(fout), p(dout), p(outs[0]), p(outs[1]) if dbias else None, p(rec), C.byref(d),
                                    R.SCALE, p(ws), 0 if ws is None else ws.numel() * 4, st)
    torch.cuda.synchronize()
    assert rc == plan['rc']
    for o in outs:
        assert bool((o == SENTINEL).all())
    assert not rec.any()


def test_rows_between_strided_units_stay_untouched(ops):
    """units with three rows of no unit between the samples (so > n_tok x pixels): those rows of out and dqkv keep what they held"""
    lib, p = ops._lib_(), ops._p
    heads, hd, n = 4, 128, 24
    lay = R.layout('temporal', 3, 5, n, pad=3)
    rows = lay[6]
    d = _desc(ops, lay, heads)
    c = dict(R.A('gaps', lay), name='gaps')
    R.A_BY_NAME['gaps'] = c
    try:
        t = R.a_inputs('gaps')
        ref = R.reference_of_a('gaps')
    finally:
        del R.A_BY_NAME['gaps']
    qkv, dout, cos, sin, bias = (dev(t[k]) for k in ('qkv', 'dout', 'cos', 'sin', 'bias'))
    out, dqkv, dbias = _filled(rows, hd), _filled(rows, 3 * hd), _filled(heads, n, n)
    nb = lib.wdno_attn_bwd_ws_bytes(C.byref(d))
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    st = ops._stream()
    assert lib.wdno_attn_fwd_amax(p(qkv), p(cos), p(sin), p(bias), p(out), None, C.byref(d), R.SCALE, st) == 0
    assert lib.wdno_attn_bwd_amax(p(qkv), p(cos), p(sin), p(bias), p(out), p(dout), p(dqkv), p(dbias), None, C.byref(d), R.SCALE, p(ws), nb, st) == 0
    used = torch.zeros(rows, dtype=torch.bool)
    used[t['idx'].reshape(-1)] = True
    assert int((~used).sum()) == 9
    free = (~used).to(DEV)
    assert bool((out[free] == SENTINEL).all()) and bool((dqkv[free] == SENTINEL).all())
    got = {'out': out.clone(), 'dqkv': dqkv.clone(), 'dbias': dbias}
    got['out'][free], got['dqkv'][free] = 0.0, 0.0
    _gate('attn', got, ref, 'gaps')


# ------------------------------------------------------------------------------------------------------------------ softmax attention as planes
def _rec_of(ops, t):
    """an amax record (every slot: max|t|) as the producer of t leaves it"""
    return torch.full((ops.AMAX_FLOATS,), float(t.abs().max()), device=DEV)


def _guarded(numel, dtype=torch.float16):
    """a pre-filled buffer of exactly `numel` elements with 4096 sentinel elements behind it: (buffer, guard)"""
    big = _filled(numel + 4096, dtype=dtype)
    return big[:numel], big[numel:]


def _planes_check(hi, lo, sc, guard, t32, bound, ref, scale, k, label):
    """the delivered planes of the tensor whose fp32 form is t32. hi, lo [rows, width] fp16 (lo, sc None: the single bf16 plane)"""
    assert bool((guard == SENTINEL).all()), label
    if lo is None:
        assert torch.equal(hi.view(torch.bfloat16), t32.bfloat16()), label
        r = R.bf16_ratio(hi.view(torch.bfloat16).double().cpu(), ref, scale, k)
        print(f'{label}: bf16 plane ratio / K {r:.3f}')
        assert r <= 1.0, (label, r)
        return
    s = float(sc)
    assert s == R.scale_from_amax(bound) and float(ref.abs().max()) <= bound, (label, s, bound)
    h, l = hi.float().cpu(), lo.float().cpu()
    assert torch.isfinite(h).all() and torch.isfinite(l).all() and float(h.abs().max()) <= 2.0 ** 15, label
    eh, el = R.planes(t32.cpu(), s)
    assert torch.equal(h, eh) and torch.equal(l, el), label
    r = R.plane_ratio(h, l, s, ref, scale, k)
    print(f'{label}: plane pair ratio / K {r:.3f}  scale 2^{math.log2(s):.0f}  max|ref| / bound {float(ref.abs().max()) / bound:.3g}')
    assert r <= 1.0, (label, r)


def _attn_dev(ops, c, t):
    lay = c['lay']
    cos, sin = dev(t['cos']), dev(t['sin'])
    return _desc(ops, lay, c['heads']), lay[6], c['heads'] * R.DH, dev(t['qkv']), cos, sin, dev(t['bias'])


@pytest.mark.parametrize('pair', [True, False], ids=['pair', 'single'])
@pytest.mark.parametrize('name', R.PA_FWD)
def test_attention_forward_planes(ops, name, pair):
    """wdno_attn_fwd_planes: |out| <= max|qkv|, `out` itself not written, the amax record that of the fp32 form"""
    lib, p = ops._lib_(), ops._p
    c, t = R.A_BY_NAME[name], R.a_inputs(name)
    d, rows, hd, qkv, cos, sin, bias = _attn_dev(ops, c, t)
    st = ops._stream()
    out32, untouched = torch.empty(rows, hd, device=DEV), _filled(rows, hd)
    (hi, guard), lo, sc = _guarded(rows * hd), (_filled(rows, hd, dtype=torch.float16) if pair else None), (_filled(1) if pair else None)
    rec32, rec = torch.zeros(ops.AMAX_FLOATS, device=DEV), torch.zeros(ops.AMAX_FLOATS, device=DEV)
    with ops._lib.debug_mode(c['debug']):
        pl = ops.attn_plan('fwd', c['heads'], *c['lay'][:6], rot=c['rot'], bias=c['bias'], planes=True)
        assert pl['rc'] == 0 and pl['family'] in ('mfma', 'mfma24', 'mfma64') and _subset(pl, c['fwd']) == c['fwd'], pl
        assert pl == ops.attn_plan('fwd', c['heads'], *c['lay'][:6], rot=c['rot'], bias=c['bias'])
        assert lib.wdno_attn_fwd_amax(p(qkv), p(cos), p(sin), p(bias), p(out32), p(rec32), C.byref(d), R.SCALE, st) == 0
        assert lib.wdno_attn_fwd_planes(p(qkv), p(cos), p(sin), p(bias), p(untouched), p(hi), p(lo), p(sc), p(rec), p(_rec_of(ops, qkv)), C.byref(d),
                                        R.SCALE, st) == 0
    torch.cuda.synchronize()
    assert bool((untouched == SENTINEL).all()) and float(rec.max()) == float(rec32.max()) == float(out32.abs().max())
    ref, scale = R.reference_of_a(name)
    _planes_check(hi.view(rows, hd), lo, sc, guard, out32, R.attn_fwd_plane_bound(t['qkv'].abs().max()), ref['out'], scale['out'], R.K['a_out'],
                  f"{name} {pl['family']} x{pl['max_walk']}")


@pytest.mark.parametrize('pair', [True, False], ids=['pair', 'single'])
@pytest.mark.parametrize('name', R.PA_BWD)
def test_attention_backward_planes(ops, name, pair):
    """wdno_attn_bwd_planes: the scale from the bound csrc/attention.hip derives of the records of qkv and dout; the bias gradient that of the fp32 form"""
    lib, p = ops._lib_(), ops._p
    c, t = R.A_BY_NAME[name], R.a_inputs(name)
    d, rows, hd, qkv, cos, sin, bias = _attn_dev(ops, c, t)
    n, heads = c['lay'][2], c['heads']
    dout = dev(t['dout'])
    st = ops._stream()
    out32, dqkv32 = torch.empty(rows, hd, device=DEV), torch.empty(rows, 3 * hd, device=DEV)
    (hi, guard), lo, sc = _guarded(rows * 3 * hd), (_filled(rows, 3 * hd, dtype=torch.float16) if pair else None), (_filled(1) if pair else None)
    db32, db = (_filled(heads, n, n), _filled(heads, n, n)) if c['dbias'] else (None, None)
    with ops._lib.debug_mode(c['debug']):
        pl = ops.attn_plan('bwd', heads, *c['lay'][:6], rot=c['rot'], bias=c['bias'], dbias=c['dbias'], planes=True)
        assert pl['rc'] == 0 and pl['family'] in ('mfma', 'mfma24') and _subset(pl, c['back']) == c['back'], pl
        nb = lib.wdno_attn_bwd_ws_bytes(C.byref(d))
        ws = torch.empty(max(nb, 4), dtype=torch.uint8, device=DEV)
        assert lib.wdno_attn_fwd_amax(p(qkv), p(cos), p(sin), p(bias), p(out32), None, C.byref(d), R.SCALE, st) == 0
        assert lib.wdno_attn_bwd_amax(p(qkv), p(cos), p(sin), p(bias), p(out32), p(dout), p(dqkv32), p(db32), None, C.byref(d), R.SCALE, p(ws), nb, st) == 0
        rq, rd = _rec_of(ops, qkv), _rec_of(ops, dout)                     # (held: two temporaries can be given the same block, one after the other)
        assert lib.wdno_attn_bwd_planes(p(qkv), p(cos), p(sin), p(bias), p(out32), p(dout), p(hi), p(lo), p(sc), p(db), p(rq), p(rd), C.byref(d),
                                        R.SCALE, p(ws), nb, st) == 0
    torch.cuda.synchronize()
    if c['dbias']:
        assert torch.equal(db, db32)
    ref, scale = R.reference_of_a(name)
    _planes_check(hi.view(rows, 3 * hd), lo, sc, guard, dqkv32, R.attn_bwd_plane_bound(n, t['qkv'].abs().max(), t['dout'].abs().max()), ref['dqkv'],
                  scale['dqkv'], R.K['a_dqkv'], f"{name} {pl['family']} x{pl['max_walk']}")


# ------------------------------------------------------------------------------------------------------------------ linear attention
def _lin_run(ops, c, t):
    qkv = dev(t['qkv'], c['bwd'])
    out = ops.linear_attention(qkv, c['units'], c['n'], c['heads'], R.SCALE)
    _, kstats, ctx = out.grad_fn.saved_tensors if c['bwd'] else (None, None, None)
    got = {'out': out.detach()}
    _record_is_exact(ops, out, 'out')
    if c['bwd']:
        got.update(kmax=kstats[..., 0].clone(), ksum=kstats[..., 1].clone(), ctx=ctx.clone())
        seen = {}
        qkv.register_hook(lambda g_: seen.__setitem__('g', g_))
        out.backward(dev(t['dout']))
        got['dqkv'] = qkv.grad
        _record_is_exact(ops, seen['g'], 'dqkv')
    return got


@pytest.mark.parametrize('name', list(R.L_BY_NAME))
def test_linear_gate(ops, name):
    c, t = R.L_BY_NAME[name], R.l_inputs(name)
    with ops._lib.debug_mode(c['debug']):
        pf, pb = ops.linattn_plan(c['units'], c['n'], c['heads']), ops.linattn_plan(c['units'], c['n'], c['heads'], backward=True)
        assert pf['rc'] == 0 and pb['rc'] == 0 and _subset(pf, c['plan']) == c['plan'] and _subset(pb, c['plan_bwd']) == c['plan_bwd'], (pf, pb)
        got = _lin_run(ops, c, t)
        again = _lin_run(ops, c, t)
    ref = R.reference_of_l(name, (pf['kstats_chunks'], pf['ctx_chunks'], pb['ctx_chunks']))
    assert torch.equal(got['kmax'].double().cpu(), ref[0]['kmax'])               # a maximum has no rounding
    _gate('lin', got, ref, name)
    for k in got:
        assert torch.equal(got[k], again[k]), k


@pytest.mark.parametrize('name', ['n256', 'uh516', 'h1-n300'])
def test_a_frame_does_not_depend_on_its_position(ops, name):
    c, t = R.L_BY_NAME[name], dict(R.l_inputs(name))
    n = c['n']
    t['qkv'], t['dout'] = t['qkv'].clone(), t['dout'].clone()
    t['qkv'][-n:], t['dout'][-n:] = t['qkv'][:n], t['dout'][:n]
    got = _lin_run(ops, c, t)
    for k in ('out', 'dqkv'):
        assert torch.equal(got[k][:n], got[k][-n:]), k
    for k in ('kmax', 'ksum', 'ctx'):
        assert torch.equal(got[k][0], got[k][-1]), k


def test_linear_backward_needs_its_whole_workspace(ops):
    lib, p = ops._lib_(), ops._p
    units, n, heads = 3, 300, 4
    qkv, dout = dev(torch.randn(units * n, 384)), dev(torch.randn(units * n, 128))
    out, kstats, ctx = torch.empty(units * n, 128, device=DEV), torch.empty(units, 128, 2, device=DEV), torch.empty(units, 4, 32, 32, device=DEV)
    st = ops._stream()
    assert lib.wdno_linattn_fwd_amax(p(qkv), p(out), p(kstats), p(ctx), None, units, n, heads, R.SCALE, st) == 0
    need = lib.wdno_linattn_ws_bytes(units, heads)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    dqkv = _filled(units * n, 384)
    assert ops.linattn_plan(units, n, heads, True, need - 1)['rc'] == -4
    assert lib.wdno_linattn_bwd_amax(p(qkv), p(dout), p(kstats), p(ctx), p(dqkv), None, p(ws), need - 1, units, n, heads, R.SCALE, st) == -4
    torch.cuda.synchronize()
    assert bool((dqkv == SENTINEL).all())
    assert lib.wdno_linattn_bwd_amax(p(qkv), p(dout), p(kstats), p(ctx), p(dqkv), None, p(ws), need, units, n, heads, R.SCALE, st) == 0
    torch.cuda.synchronize()
    assert not bool((dqkv == SENTINEL).any())


@pytest.mark.parametrize('pair', [True, False], ids=['pair', 'single'])
@pytest.mark.parametrize('name', R.PL)
def test_linear_planes(ops, name, pair):
    """wdno_linattn_fwd_planes (|out| <= scale max|qkv|; the chunk partials of the context pass through the hi plane, which has exactly the room
    at one head and n_tok = 128 k) and wdno_linattn_bwd_planes (the bound uses max|dctx|, which the call measures into rec_dctx)."""
    lib, p = ops._lib_(), ops._p
    c, t = R.L_BY_NAME[name], R.l_inputs(name)
    units, n, heads = c['units'], c['n'], c['heads']
    rows, hd = units * n, heads * R.DH
    pf, pb = ops.linattn_plan(units, n, heads), ops.linattn_plan(units, n, heads, backward=True)
    assert pf['rc'] == 0 and pb['rc'] == 0 and pf['family'] == 'mfma' and _subset(pf, c['plan']) == c['plan'] and _subset(pb, c['plan_bwd']) == c['plan_bwd'], (pf, pb)
    qkv, dout = dev(t['qkv']), dev(t['dout'])
    st = ops._stream()
    new = lambda: (torch.empty(units, hd, 2, device=DEV), torch.empty(units, heads, 32, 32, device=DEV))
    (ks32, ctx32), (ks, ctx) = new(), new()
    out32, dqkv32 = torch.empty(rows, hd, device=DEV), torch.empty(rows, 3 * hd, device=DEV)
    (hi, guard), lo, sc = _guarded(rows * hd), (_filled(rows, hd, dtype=torch.float16) if pair else None), (_filled(1) if pair else None)
    (ghi, gguard), glo, gsc = _guarded(rows * 3 * hd), (_filled(rows, 3 * hd, dtype=torch.float16) if pair else None), (_filled(1) if pair else None)
    need = lib.wdno_linattn_ws_bytes(units, heads)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    rec_dctx = torch.zeros(ops.AMAX_FLOATS, device=DEV)
    rq, rd = _rec_of(ops, qkv), _rec_of(ops, dout)
    assert lib.wdno_linattn_fwd_amax(p(qkv), p(out32), p(ks32), p(ctx32), None, units, n, heads, R.SCALE, st) == 0
    assert lib.wdno_linattn_fwd_planes(p(qkv), p(hi), p(lo), p(sc), p(ks), p(ctx), p(rq), units, n, heads, R.SCALE, st) == 0
    assert lib.wdno_linattn_bwd_amax(p(qkv), p(dout), p(ks), p(ctx), p(dqkv32), None, p(ws), need, units, n, heads, R.SCALE, st) == 0
    assert lib.wdno_linattn_bwd_planes(p(qkv), p(dout), p(ks), p(ctx), p(ghi), p(glo), p(gsc), p(rq), p(rd), p(rec_dctx), p(ws), need, units, n, heads,
                                       R.SCALE, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(ks, ks32) and torch.equal(ctx, ctx32)
    ref = R.reference_of_l(name, (pf['kstats_chunks'], pf['ctx_chunks'], pb['ctx_chunks']))
    assert torch.equal(ks[..., 0].double().cpu(), ref[0]['kmax'])
    _gate('lin', {'ksum': ks[..., 1], 'ctx': ctx}, ref, name)
    a, g = t['qkv'].abs().max(), t['dout'].abs().max()
    label = f"{name} ctx chunks {pf['ctx_chunks']} / {pb['ctx_chunks']}"
    _planes_check(hi.view(rows, hd), lo, sc, guard, out32, R.lin_fwd_plane_bound(a), ref[0]['out'], ref[1]['out'], R.K['l_out'], label + ' out')
    dmax = float(rec_dctx.max())
    if pair:                                                              # (the single plane has no scale: the call does not measure dctx)
        dctx = ws[:units * heads * 4096].view(torch.float32)
        assert dmax == float(dctx.abs().max()) and dmax > 0
    _planes_check(ghi.view(rows, 3 * hd), glo, gsc, gguard, dqkv32, R.lin_bwd_plane_bound(a, g, dmax), ref[0]['dqkv'], ref[1]['dqkv'], R.K['l_dqkv'],
                  label + ' dqkv')


# ------------------------------------------------------------------------------------------------------------------ channel LayerNorm
def _ln_run(ops, c, t):
    x, g = dev(t['x'], True), dev(t['g'], True)
    if c['add']:
        y, xs = ops.layernorm_cl_skip(x, g)
    else:
        y, xs = ops.layernorm_cl(x, g), None
    _record_is_exact(ops, y, 'y')
    seen = {}
    x.register_hook(lambda g_: seen.__setitem__('g', g_))
    if c['add']:
        torch.autograd.backward([y, xs], [dev(t['dy']), dev(t['add'])])
    else:
        y.backward(dev(t['dy']))
    _record_is_exact(ops, seen['g'], 'dx')
    return {'y': y.detach(), 'dx': x.grad, 'dg': g.grad}


@pytest.mark.parametrize('name', list(R.N_BY_NAME))
def test_layernorm_gate(ops, name):
    c, t = R.N_BY_NAME[name], R.n_inputs(name)
    pl = ops.layernorm_plan(c['p'], c['c'])
    tpr, vpl = R.ln_shape(c['c'])
    assert pl['rc'] == 0 and (pl['tpr'], pl['vpl'], pl['rows_per_block'], pl['max_rows_walk']) == (tpr, vpl, 256 // tpr, c['walk']), pl
    got, again = _ln_run(ops, c, t), _ln_run(ops, c, t)
    _gate('ln', got, R.reference_of_n(name), name)
    for k in got:
        assert torch.equal(got[k], again[k]), k


def test_a_row_does_not_depend_on_the_block_or_pass_that_handled_it(ops):
    c = R.N_BY_NAME['c16-p65539-noadd-gauss-gauss']
    t = dict(R.n_inputs(c['name']))
    t['x'], t['dy'] = t['x'].clone(), t['dy'].clone()
    t['x'][-1], t['dy'][-1] = t['x'][0], t['dy'][0]
    got = _ln_run(ops, c, t)
    assert torch.equal(got['y'][0], got['y'][-1]) and torch.equal(got['dx'][0], got['dx'][-1])


@pytest.mark.parametrize('c', [1028, 6])
def test_layernorm_refusals_write_nothing(ops, c):
    lib, p = ops._lib_(), ops._p
    rows = 5
    assert ops.layernorm_plan(rows, c)['rc'] == -3
    x, g, dy = dev(torch.randn(rows, c)), dev(torch.randn(c)), dev(torch.randn(rows, c))
    y, dx, dg, rec = _filled(rows, c), _filled(rows, c), _filled(c), torch.zeros(ops.AMAX_FLOATS, device=DEV)
    ws = _filled(1024 * c)
    st = ops._stream()
    assert lib.wdno_layernorm_fwd_amax(p(x), p(g), p(y), p(rec), rows, c, R.EPS, st) == -3
    assert lib.wdno_layernorm_bwd_add_amax(p(x), p(g), p(dy), None, p(dx), p(dg), p(rec), rows, c, R.EPS, p(ws), ws.numel() * 4, st) == -3
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in (y, dx, dg, ws)) and not rec.any()


@pytest.mark.parametrize('pair', [True, False], ids=['pair', 'single'])
@pytest.mark.parametrize('c,p', [(8, 129), (96, 9), (128, 7), (256, 5), (512, 3), (1024, 4099)])
def test_layernorm_planes(ops, c, p, pair):
    """y delivered as planes. Pair: the scale is the one the documented bound |y| <= sqrt(C) max|g| implies, no entry saturates, and hi / s + lo / s
    is held to the fp64 reference with the split's own rounding added to the gate: the lo plane carries 11 bits below the hi plane's 11
    (2^-22 |y|) and is sub-normal below 2^-14 (2^-25 / s). Single bf16 plane: in units of 2^-9, held to 2 of them: bf16 keeps 8 significant bits, round to nearest
    is off by half an ulp, and an ulp is at most 2^-7 |y|."""
    lib, ptr = ops._lib_(), ops._p
    name = next(k for k, v in R.N_BY_NAME.items() if v['c'] == c and v['p'] == p)
    t = R.n_inputs(name)
    (out, scale) = R.reference_of_n(name)
    x, g = dev(t['x']), dev(t['g'])
    hi = _filled(p, c, dtype=torch.float16)
    lo, sc = (_filled(p, c, dtype=torch.float16), _filled(1)) if pair else (None, None)
    assert lib.wdno_layernorm_fwd_planes(ptr(x), ptr(g), ptr(hi), ptr(lo), ptr(sc), p, c, R.EPS, ops._stream()) == 0
    y, s_y = out['y'], scale['y']
    if not pair:
        got = hi.view(torch.bfloat16).double().cpu()
        assert bool(((got - y).abs() <= 2 * 2.0 ** -9 * y.abs() + R.K['n_y'] * R.U * s_y + 2.0 ** -126).all())
        return
    s = float(sc)
    bound = float(torch.tensor(math.sqrt(c), dtype=torch.float32) * t['g'].abs().max())
    assert s == scale_from_amax(bound) and float(y.abs().max()) <= bound
    h, l = hi.double().cpu(), lo.double().cpu()
    assert float(h.abs().max()) < 2.0 ** 15 and torch.isfinite(h).all() and torch.isfinite(l).all()
    err = ((h + l) / s - y).abs()
    assert bool((err <= R.K['n_y'] * R.U * s_y + 2.0 ** -22 * y.abs() + 2.0 ** -25 / s).all()), float((err / (R.U * s_y)).max())


@pytest.mark.parametrize('c', [12, 36, 260])
def test_layernorm_planes_refuse_channels_that_are_no_multiple_of_eight(ops, c):
    """include/wdno_hip.h: the fp32 form takes C % 4 == 0, the planes form C % 8 == 0 only; refused before any launch, nothing written"""
    lib, ptr = ops._lib_(), ops._p
    rows = 5
    assert ops.layernorm_plan(rows, c)['rc'] == 0
    x, g = dev(torch.randn(rows, c)), dev(torch.randn(c))
    hi, lo, sc = _filled(rows, c + 4, dtype=torch.float16), _filled(rows, c + 4, dtype=torch.float16), _filled(1)
    assert lib.wdno_layernorm_fwd_planes(ptr(x), ptr(g), ptr(hi), ptr(lo), ptr(sc), rows, c, R.EPS, ops._stream()) == -3
    assert lib.wdno_layernorm_fwd_planes(ptr(x), ptr(g), ptr(hi), None, None, rows, c, R.EPS, ops._stream()) == -3
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in (hi, lo, sc))
