"""tests/conv_ref.py checked on the CPU: the references against F.conv*d and autograd, the exactness condition of every (case, family,
pass) of the exact gate, the fp32 transcription against K / 2, every case's launch plan against the library's plan queries (which launch
nothing and answer for 256 CUs without a device), and the Python profiling-key mirrors of wdno_amd/ops.py against the same queries."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as R

IDS = [c.name for c in R.CASES]
LIMIT = 2.0 ** 24


@pytest.fixture(scope='module')
def ops():
    from wdno_amd import ops as o
    o._lib_()
    return o


def _h3(case):
    return case.plan[0] is not None


def test_matrix_is_well_formed():
    assert len(set(IDS)) == len(IDS)
    for c in R.CASES:
        assert c.plan is not None and len(c.plan) == 3, c.name
        assert all(p is None for p in c.plan) or all(p is not None for p in c.plan), c.name       # int2 needs every pass on split kernels
        assert sum(1 for o in R.CASES if R.data_key(o) == R.data_key(c)) <= 2
    for fam in ('fp32', 'h3', 'h3d', 'h3t', 'h3t_stem'):          # every forward family and every weight-gradient family is visited
        assert any(fam == (c.plan[0] or 'fp32:').split(':')[0] for c in R.CASES), fam
    for fam in R.WGRAD_FAMILY:
        assert any(c.plan[2] and c.plan[2].startswith(fam + ':') for c in R.CASES), fam


@pytest.mark.parametrize('case', R.CASES, ids=IDS)
def test_case_reaches_its_plan(ops, case):
    """The regime each case exists for, from the library's own choosing code at its 256-CU answer, under the case's debug mode."""
    with ops._lib.debug_mode(case.mode):
        got = R.plans(ops, case)
    assert got == case.plan, (case.name, got, case.plan)
    assert (got[0] is None) == (not ops._use_h3(math.prod(R.dims(case)[-1]) * case.xs[0], ops.pad4(case.xs[1]) * math.prod(R.dims(case)[4])))


def test_split_is_refused_without_workspace(ops):
    """The four-run split needs the caller's workspace: with none, or too small a one, the plan is the unsplit 64 x 64 kernel."""
    import ctypes as C
    case = R.BY_NAME['split4_residual']
    (_, _, g, _), = [l for l in R.launches(ops, case) if l[0] == 'y']
    need = int(ops._lib_().wdno_conv_fwd_split_ws_bytes(C.byref(g)))
    assert need == 4 * 1024 * 256 * 4
    assert R.fwd_plan_str(ops.conv_fwd_plan(g, False, False, need)) == 'h3t:128x128/4 t16 g64'
    for ws in (0, need - 1):
        assert R.fwd_plan_str(ops.conv_fwd_plan(g, False, False, ws)) == 'h3t:64x64 t64 g64'
    assert R.fwd_plan_str(ops.conv_fwd_plan(g, True, False, 0)) == 'h3t:64x64 t64 g64'             # single bf16 planes: their entry points lend no workspace
    assert R.fwd_plan_str(ops.conv_fwd_plan(g, None)) == 'fp32:64x64 t64 g64'                      # the exact-fp32 entry point's own tile


def test_residual_that_is_y_itself_refuses_the_two_block_form(ops):
    """The only way a residual changes the choice: accumulation in place cannot take the ksplit form, which adds onto zeroed outputs."""
    case = R.BY_NAME['reg_64x64_ksplit2']
    (_, _, g, _), = [l for l in R.launches(ops, case) if l[0] == 'y']
    assert R.fwd_plan_str(ops.conv_fwd_plan(g, False, False)) == 'h3:64x64k2 t32 g32' == case.plan[0]
    assert R.fwd_plan_str(ops.conv_fwd_plan(g, False, True)) == 'h3:64x64 t32 g32'


def test_stem_weight_gradient_has_two_splits_from_1024_pixels_on(ops):
    """splits == 1 of the stem weight gradient needs at most 512 pixels, which ops.conv_cl sends to the exact-fp32 kernels: the device
    test of that path builds its planes itself."""
    assert ops.H3_MIN_PIXELS == 1024
    for taps in ((1, 1), (3, 3), (7, 7), (8, 8)):
        for n in list(range(2, 40)) + [64, 100, 1000]:
            sp = (1, 16, 32)
            g = ops._geom((n, *sp), 48, 16, (*taps, 7), (1, 1, 1), (taps[0] // 2, taps[1] // 2, 3), sp)
            if taps[0] % 2 == 0:
                continue                                  # (even taps do not keep the grid)
            pl = ops.conv_wgrad_plan(g, False, 16, 42)
            assert R.WGRAD_FAMILY[pl.family] == 'h3s' and pl.splits >= 2, (taps, n, pl.splits)
    g = ops._geom((1, 2, 16, 16), 48, 16, (3, 3, 7), (1, 1, 1), (1, 1, 3), (2, 16, 16))
    assert R.wgrad_plan_str(ops.conv_wgrad_plan(g, False, 16, 42)).startswith('h3s:64x352 s1 ')


def test_single_plane_plans(ops):
    """Single bf16 planes: the wide 256 x 128 tap-resident tiles from two rounds of them on, the 256-pixel stem tiles always."""
    g = ops._geom((64, 1, 64, 64), 32, 128, (1, 3, 3), (1, 1, 1), (0, 1, 1), (1, 64, 64))
    assert R.fwd_plan_str(ops.conv_fwd_plan(g, True)) == 'h3t:256x128 t1024 g256'
    assert R.fwd_plan_str(ops.conv_fwd_plan(g, False)).startswith('h3t:') and '256x128' not in R.fwd_plan_str(ops.conv_fwd_plan(g, False))
    case = R.BY_NAME['stem_2d_natural']
    (_, _, g, _), = [l for l in R.launches(ops, case) if l[0] == 'y']
    assert R.fwd_plan_str(ops.conv_fwd_plan(g, True)) == 'h3t_stem:256x64 t100 g100'
    assert R.fwd_plan_str(ops.conv_fwd_plan(g, False)) == 'h3t_stem:192x64 t134 g134'


@pytest.mark.parametrize('case', R.CASES, ids=IDS)
def test_profiling_keys_agree_with_the_library(ops, case):
    """ops._fwd_h3_kernel_name / _wgrad_h3_kernel_name (bench.py's profiling keys) are Python re-statements of the C++ dispatch: on every
    launch of the matrix they must name the kernel family and tile the library's plan names."""
    with ops._lib.debug_mode(0):          # the mirrors know nothing of debug modes
        for name, kind, g, extra in R.launches(ops, case):
            ks, pixels = (g.kd, g.kh, g.kw), g.N * g.OD * g.OH * g.OW
            if kind == 'fwd':
                lowp, has_res = extra
                pl = R.plan_of(ops, kind, g, extra).split()[0]
                fam, tile = pl.split(':')
                tap = ((g.YD, g.YH, g.YW, g.osd, g.osh, g.osw) == (g.OD, g.OH, g.OW, 1, 1, 1) and (g.sd, g.sh, g.sw) == (1, 1, 1) and
                       (g.OD, g.OH, g.OW) == (g.D, g.H, g.W) and max(ks) <= 8 and ((g.kw == 3 and g.C % 32 == 0) or (g.kw == 7 and g.C % 16 == 0 and g.K <= 64)))
                key = ops._fwd_h3_kernel_name(pixels, g.K, ks, tap, g.C)
                if fam == 'h3':
                    assert key == ('conv_fwd_h3_kernel<..,128>' if g.K > 64 else 'conv_fwd_h3_kernel<..,64>'), (case.name, name, key, pl)
                else:
                    bm, bn = tile.rstrip('ul').split('/')[0].split('x')
                    want = f'conv_fwd_h3{"d" if fam == "h3d" else "t"}_kernel<{bm},{bn}>' + ('/4' if '/4' in tile else '')
                    assert key == want, (case.name, name, key, pl)
            else:
                pl = R.plan_of(ops, kind, g, extra).split()[0]
                fam, tile = pl.split(':')
                window = (g.sd, g.sh, g.sw) == (1, 1, 1) and (g.OD, g.OH, g.OW) == (g.D, g.H, g.W) and g.kw == 3 and g.pw == 1 and g.C % 64 == 0
                if (g.sd, g.sh, g.sw) == (1, 1, 1) and (g.OD, g.OH, g.OW) == (g.D, g.H, g.W) and g.kw == 7 and g.pw == 3 and g.C == 48 and g.K <= 64 and max(ks) <= 8:
                    window = 'stem'
                key = ops._wgrad_h3_kernel_name(g.K, g.kw * g.C, window)
                bm, bn = tile.split('x')
                # (in production the register-staged weight gradient runs only where the DMA kernels refuse a size: the key names the DMA kernel)
                assert fam in ('h3d', 'h3w', 'h3s'), (case.name, name, 'no profiling key is defined for a production weight gradient of family', fam)
                want = {'h3d': f'conv_wgrad_h3d_kernel<{bm},{bn}>', 'h3w': 'conv_wgrad_h3w_kernel<64,384>', 'h3s': 'conv_wgrad_h3s_kernel<64,352>'}[fam]
                assert key == want, (case.name, name, key, pl)


SMALL = [c for c in R.CASES if R.reduction_lengths(c)['dw'] * R.reduction_lengths(c)['y'] * c.ws[0] <= 3e8]


@pytest.mark.parametrize('case', SMALL, ids=[c.name for c in SMALL])
def test_reference_is_torch_autograd(case):
    """reference() against one autograd graph of F.conv*d with bias and residual, in fp64."""
    t = R.inputs(case, 'gauss')
    nd = len(case.ws) - 2
    conv = (F.conv3d, F.conv2d)[3 - nd]
    leaves = {k: v.double().clone().requires_grad_(True) for k, v in t.items() if v is not None and k != 'dy'}
    y = conv(leaves['x'], leaves['w'], leaves.get('bias'), stride=case.stride, padding=case.padding)
    if 'res' in leaves:
        y = y + leaves['res']
    y.backward(t['dy'].double())
    ref = R.reference(t, case)
    want = {'y': y.detach(), 'dx': leaves['x'].grad + (t['skip'].double() if case.skip else 0), 'dw': leaves['w'].grad}
    if case.bias:
        want['db'] = leaves['bias'].grad
    if case.residual:
        want['dres'] = leaves['res'].grad
    assert want.keys() == ref.keys()
    for k, v in want.items():
        assert float((ref[k] - v).abs().max()) <= 1e-12 * float(v.abs().max()), (case.name, k)


def test_planes_emulation():
    """plane_pack in torch: the scale puts amax in [2^14, 2^15); the int2 values split into +-2^14 and 4 b, also at the tie 16380."""
    v = torch.tensor([4097.0, 4096.0, 4095.0, -4095.0, -4097.0, 0.0, 4096.0])
    hi, lo, s = R.planes(v)
    assert s == 4.0
    assert hi.tolist() == [16384.0, 16384.0, 16384.0, -16384.0, -16384.0, 0.0, 16384.0]
    assert lo.tolist() == [4.0, 0.0, -4.0, 4.0, -4.0, 0.0, 0.0]
    hi, lo, s = R.planes(torch.tensor([4.0, -3.0, 1.0, 0.0]))
    assert s == 4096.0 and lo.abs().max() == 0 and hi.tolist() == [16384.0, -12288.0, 4096.0, 0.0]
    g = torch.tensor([1.0, 1e-3, -0.7, 3e-6, 1.9999])
    hi, lo, s = R.planes(g)
    assert 2.0 ** 14 <= 1.9999 * s < 2.0 ** 15
    assert float(((hi + lo) / s - g.double()).abs().max()) <= 2.0 ** -21 * 1.9999


@pytest.mark.parametrize('case', R.CASES, ids=IDS)
def test_exactness_conditions_hold(case):
    """Every (case, family, pass) of the exact gate: sum |terms| below 2^24 units, hi + lo == v s, and the planes form equal to the plain
    fp64 convolution (int1) or to conv(x, w) - conv(bx, bw) (int2). The expected tensors are then exactly representable in fp32."""
    for family in ('int1', 'int2') if _h3(case) else ('int1',):
        t = R.inputs(case, family)
        worst, rec = R.exactness(t, case, family)
        assert rec, (case.name, family)
        for name, v in worst.items():
            assert v < LIMIT, (case.name, family, name, v / LIMIT)
        pr = R.planes_reference(t, case)
        ref = R.reference(t, case)
        if family == 'int2':
            low = lambda v: None if v is None else torch.where(v == 0, v, v - torch.sign(v) * 4096.0)
            tb = dict(t, x=low(t['x']), w=low(t['w']), bias=None, res=None, skip=None)
            cross = R.reference(tb, case)                      # conv(bx, bw): the al bl products the kernels leave out
            tg = dict(tb, dy=low(t['dy']))
            ref = dict(ref, y=ref['y'] - cross['y'], dx=ref['dx'] - R.reference(dict(tg, x=t['x']), case)['dx'],
                       dw=ref['dw'] - R.reference(dict(tg, w=t['w']), case)['dw'])
        for name in pr:
            assert torch.equal(pr[name], ref[name]), (case.name, family, name)
            assert torch.equal(pr[name].float().double(), pr[name]), (case.name, family, name)       # one rounding to fp32 changes nothing
        if family == 'int2':                                   # the lo planes and the tie really occur
            assert float(t['x'].abs().max()) == 4097.0 and (t['x'].abs() == 4095.0).any() and (t['w'].abs() == 4095.0).any()


MEASURED = {}


@pytest.mark.parametrize('case', R.CASES, ids=IDS)
def test_transcription_stays_within_half_the_gate(case):
    """K is ceil(4 x the fp32 transcription's worst ratio): the transcription itself is held to K / 2 on every case and family."""
    for family in [f for f in R.families(case) if f in ('gauss', 'range')]:
        t = R.inputs(case, family)
        ref, scale, flush = R.expected(case, family)
        got = R.transcription(t, case)
        for name in ('y', 'dx', 'dw', 'db'):
            if name not in got:
                continue
            r = R.ratio(got[name], ref[name], scale[name], flush[name])
            cls = (name, 'long' if R.reduction_lengths(case)[name] >= R.LONG else 'short')
            MEASURED[cls] = max(MEASURED.get(cls, 0.0), r)
            print(f'{case.name} {family} {name}: {r:.2f} / {R.k_of(case, name)}   worst so far {cls}: {MEASURED[cls]:.2f}')
            assert r <= R.k_of(case, name) / 2, (case.name, family, name, r)
        if 'dres' in got:
            assert torch.equal(got['dres'], t['dy'])


def test_the_gates_see_a_missing_product():
    """Half the channels of one output pixel computed without their xl wh products: the exact gate fails at exactly that pixel, the
    element-wise gate at some of its elements, and the whole-tensor rel-L2 the older tests use stays below their 2e-6 bar."""
    case = R.BY_NAME['tap_64x64']
    for family in ('int2', 'gauss'):
        t = R.inputs(case, family)
        (xh, xl, sx), (wh, wl, sw) = R.planes(t['x']), R.planes(t['w'])
        good = (R._conv(xh, wh + wl, case) + R._conv(xl, wh, case)) / (sx * sw)
        bad = good.clone()
        bad[1, :32, 7, 5] = (R._conv(xh, wh + wl, case) / (sx * sw))[1, :32, 7, 5]
        b = t['bias'].double().reshape(1, -1, 1, 1)
        if family == 'int2':
            want = R.expected(case, family)['y']
            assert torch.equal((good + b).float(), want)
            wrong = ((bad + b).float() != want).nonzero()
            assert wrong.numel() and set(wrong[:, 0].tolist()) == {1} and set(wrong[:, 2].tolist()) == {7} and set(wrong[:, 3].tolist()) == {5}
            assert 'rows(h) [7] columns(w) [5]' in R.wrong_elements((bad + b).float(), want, 'y', case)
        else:
            ref, scale, flush = R.expected(case, family)
            assert R.ratio((good + b).float(), ref['y'], scale['y'], flush['y']) <= R.k_of(case, 'y')
            assert R.ratio((bad + b).float(), ref['y'], scale['y'], flush['y']) > 4 * R.k_of(case, 'y')
            rel = float(((bad + b) - ref['y']).norm() / ref['y'].norm())
            assert rel < 2e-6, rel


@pytest.mark.parametrize('case,plan', R.BF16_CASES, ids=[c.name for c, _ in R.BF16_CASES])
def test_single_plane_subset(ops, case, plan):
    """Single bf16 planes: the plan of every case, int1 exact on one plane (the planes form equals the plain convolution), and the
    one-plane transcription within K16 / 2 of the 2^-9 gate."""
    with ops._lib.debug_mode(case.mode):
        assert R.plans(ops, case, lowp=True) == plan
    t = R.inputs(case, 'int1')
    assert float(max(t[k].abs().max() for k in ('x', 'w', 'dy'))) == 4.0          # exact in bf16
    pr, ref = R.planes_reference(t, case, single=True), R.reference(t, case)
    assert all(torch.equal(pr[k], ref[k]) for k in ref)
    t = R.inputs(case, 'gauss')
    ref, scale, flush = R.expected(case, 'gauss')
    got = R.transcription(t, case, single=True)
    for name, k in R.K16.items():
        r = R.ratio(got[name], ref[name], scale[name], None, R.U16)
        print(f'{case.name} bf16 {name}: {r:.2f} / {k}')
        assert r <= k / 2, (case.name, name, r)


@pytest.mark.parametrize('family', ['int1', 'int2'])
def test_conv_transpose_exactness(family):
    """The transposed convolution's exact inputs: the condition holds, and the planes form is the plain fp64 result (int1)."""
    t = R.convt_inputs(family)
    for name, v in R.convt_exactness(t, family).items():
        assert v < LIMIT, (family, name, v / LIMIT)
    pr = R.convt_reference(t, True)
    for name, v in pr.items():
        assert torch.equal(v.float().double(), v), (family, name)
    if family == 'int1':
        ref = R.convt_reference(t, False)
        assert all(torch.equal(pr[k], ref[k]) for k in ref)
