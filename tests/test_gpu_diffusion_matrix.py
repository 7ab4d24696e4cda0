"""The kernels of csrc/diffusion.hip held ELEMENT BY ELEMENT to the fp64 reference of tests/diffusion_kernels_ref.py, |got - ref| <= K 2^-24 S_e
(K per output: the roundings on its path plus one, derived there and anchored on the CPU by tests/test_host_diffusion_kernels_ref.py; S_e the
same formula on absolute values; exact where S_e = 0), on a case matrix chosen by launch form: every operation in its scalar and its float4
form, every reason for the scalar form (W, inner or per_sample not a multiple of 4, each operand in turn at a 4-byte offset, nb < B, B > 2048,
B > 65535), a second ragged grid-stride round, every flag combination of both condition trees, the fused-gradient arm, gscale given and NULL,
noise and x_start NULL, clamp on and off. Per case: the plan query names the form and the grid; the entry points are called through ctypes on
views into sentinel-filled allocations (guard bands untouched, inputs unchanged, every output element written); a second run gives equal bits;
the exact-bit requirements hold (clean -> the source's bits, zero -> +0, the target the noise's bits or +0, untouched elements of apply_cond,
clamped x_start in [-1, 1], DDIM-dev == DDIM); the wrappers of wdno_amd.diffusion_core give the bits of the direct calls. Where a case exists
for a 4-byte offset, the aligned (float4) launch on the same values gives EQUAL BITS for every element-wise output: a result does not depend
on alignment (the build compiles with -ffp-contract=off, so both forms are the same sequence of IEEE operations per element). The scalar loss
is not pinned that way: the two forms add their partial sums in different orders."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests import diffusion_kernels_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def env():
    from wdno_amd import diffusion_core as K
    from wdno_amd import ops
    return types.SimpleNamespace(K=K, ops=ops, lib=ops._lib_(), p=ops._p, stream=ops._stream)


# ------------------------------------------------------------------------------------------------------------------ sentinel-filled operands
class Operand:
    """n floats inside a larger allocation filled with SENTINEL: GUARD floats before and after, one float further in for a 4-byte offset. An
    input holds `data`; an output holds the UNWRITTEN pattern until the launch."""

    def __init__(self, n, data=None, misalign=False, dtype=torch.float32):
        self.n, self.off = n, R.GUARD + (1 if misalign else 0)
        self.arena = torch.full((R.GUARD + n + R.GUARD + 4,), R.SENTINEL, device=DEV, dtype=dtype)
        self.v = self.arena[self.off:self.off + n]
        assert self.v.data_ptr() % 16 == (4 if misalign else 0)
        self.data = None if data is None else torch.from_numpy(np.ascontiguousarray(data).reshape(-1)).to(DEV)
        if self.data is not None:
            self.v.copy_(self.data)
        elif dtype == torch.float32:
            self.v.view(torch.int32).fill_(R.UNWRITTEN)

    @property
    def ptr(self):
        return self.v.data_ptr()

    def check(self, what, written=True):
        a = self.arena
        assert bool((a[:self.off] == R.SENTINEL).all()) and bool((a[self.off + self.n:] == R.SENTINEL).all()), f'{what}: guard band written'
        if self.data is not None:
            assert torch.equal(self.v.view(torch.int32), self.data.view(torch.int32)), f'{what}: input changed'
        elif a.dtype != torch.float32:                                                    # the fp64 workspace: scratch, only a refused call is checked
            assert written or bool((self.v == R.SENTINEL).all()), f'{what}: written by a refused call'
        elif written:
            assert bool((self.v.view(torch.int32) != R.UNWRITTEN).all()), f'{what}: output element not written'
        else:
            assert bool((self.v.view(torch.int32) == R.UNWRITTEN).all()), f'{what}: output written by a refused call'

    def numpy(self, shape):
        return self.v.cpu().numpy().reshape(shape).copy()


def _mask(*ops_):
    m = 0
    for o in ops_:
        if o is not None:
            m |= o.ptr
    return m


def _ptr(o):
    return None if o is None else o.ptr


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _same(a, b):
    return np.array_equal(R.bits(a), R.bits(b))


def _report(family, form, output, r, k, name):
    print(f'RATIO {family} {form} {output} {r / k:.3f} K={k} {name}')


# ------------------------------------------------------------------------------------------------------------------ conditions
def _schedule(c):
    b = R.tables('sigmoid' if c['tree'] == 0 else 'cosine')
    return b['sqrt_alphas_cumprod'], b['sqrt_one_minus_alphas_cumprod']


def _run_q(env, c, i, desc, mis, expect):
    sa, sb = _schedule(c)
    n = c['total']
    x0, nz = Operand(n, i['x0'], mis == 'x0'), Operand(n, i['noise'], mis == 'noise')
    xo, to = Operand(n, misalign=mis == 'x'), Operand(n, misalign=mis == 'target')
    p = env.K.cond_plan(desc, _mask(x0, nz, xo, to))
    assert p['rc'] == 0 and R.plan_tuple(p) == expect, p
    t, sa_d, sb_d = _dev(i['t']), _dev(sa), _dev(sb)
    rc = env.lib.wdno_q_sample_cond(x0.ptr, nz.ptr, env.p(t), env.p(sa_d), env.p(sb_d), xo.ptr, to.ptr, C.byref(desc), env.stream())
    assert rc == 0
    for o, w in ((x0, 'x0'), (nz, 'noise'), (xo, 'x'), (to, 'target')):
        o.check(f'q_sample_cond {w}')
    return xo.numpy(c['shape']), to.numpy(c['shape'])


def _run_apply(env, c, i, desc, mis, expect):
    n = c['total']
    x, src = Operand(n, i['x'], mis in ('x0', 'x')), Operand(n, i['x0'], mis in ('noise', 'target'))
    p = env.K.cond_plan(desc, _mask(x, src))
    assert p['rc'] == 0 and R.plan_tuple(p) == expect, p
    assert env.lib.wdno_apply_cond(x.ptr, src.ptr, C.byref(desc), env.stream()) == 0
    x.data = None
    x.check('apply_cond x', written=True)
    src.check('apply_cond src')
    return x.numpy(c['shape'])


@pytest.mark.parametrize('name', list(R.COND_BY_NAME))
def test_cond_gate(env, name):
    c = R.COND_BY_NAME[name]
    K = env.K
    i = R.cond_inputs(c)
    desc = R.cond_desc_of(K, c)
    sa, sb = _schedule(c)
    for p in R.cond_plans(K, c).values():                                                 # 1. the form and the grid the case states
        assert p['rc'] == 0 and R.plan_tuple(p) == c['expect'], p
    ref = R.cond_reference(c, i['x0'], i['noise'], i['t'], sa, sb)
    x, tgt = _run_q(env, c, i, desc, c['misalign'], c['expect'])                           # 2. run: guard bands, inputs, every element written
    x2, tgt2 = _run_q(env, c, i, desc, c['misalign'], c['expect'])
    assert _same(x, x2) and _same(tgt, tgt2), 'second run'                                 # 3. again
    r = R.ratio(x, ref['x'], ref['x_scale'])                                               # 4. the gate
    _report('cond', c['expect'][0], 'x', r, R.K_Q, name)
    assert r <= R.K_Q, r
    code = ref['code']                                                                     # 5. exact bits
    assert np.array_equal(R.bits(x)[code == 2], R.bits(i['x0'])[code == 2]), 'clean: the source bits'
    assert not R.bits(x)[code == 1].any(), 'zero: +0'
    assert np.array_equal(R.bits(tgt), R.bits(ref['target'])), 'target: the noise bits or +0'
    a = _run_apply(env, c, i, desc, c['misalign'], c['expect'])                            # 6. apply_cond: exact everywhere
    a2 = _run_apply(env, c, i, desc, c['misalign'], c['expect'])
    assert _same(a, a2), 'apply_cond second run'
    assert np.array_equal(R.bits(a), R.bits(R.apply_reference(c, i['x'], i['x0'], code)))
    if c['misalign']:                                                                      # 7. the same bits whatever the alignment
        aligned = ('float4', R.grid1(c['total'] // 4), 1)
        xa, ta = _run_q(env, c, i, desc, None, aligned)
        assert _same(x, xa) and _same(tgt, ta) and _same(a, _run_apply(env, c, i, desc, None, aligned)), 'scalar against float4'
        print(f'PIN cond {name}: scalar == float4')
    elif not name.startswith('rounds'):                                                    # 8. the wrappers
        xw, tw = K.q_sample_cond(_dev(i['x0']), _dev(i['noise']), _dev(i['t']), _dev(sa), _dev(sb), desc)
        aw = K.apply_cond(_dev(i['x']), _dev(i['x0']), desc)
        assert _same(xw.cpu().numpy(), x) and _same(tw.cpu().numpy(), tgt) and _same(aw.cpu().numpy(), a), 'wrapper'


def test_check_cond_refusals(env):
    """tree = 2, tree = 1 with F != 1, a zero extent: WDNO_EINVAL from both entry points, and nothing is written"""
    from wdno_amd._lib import CondDesc
    c = R.COND_BY_NAME['smoke-w8-C42-pad']
    i = R.cond_inputs(c)
    ok = R.cond_desc_of(env.K, c)
    sa, sb = _schedule(c)
    t, sa_d, sb_d = _dev(i['t']), _dev(sa), _dev(sb)
    n = c['total']
    for edit in (dict(tree=2), dict(tree=1), dict(H=0), dict(B=0)):
        d = CondDesc.from_buffer_copy(bytes(ok))
        for k, v in edit.items():
            setattr(d, k, v)
        assert d.tree != 1 or d.F != 1
        x0, nz, xo, to = Operand(n, i['x0']), Operand(n, i['noise']), Operand(n), Operand(n)
        assert env.lib.wdno_q_sample_cond(x0.ptr, nz.ptr, env.p(t), env.p(sa_d), env.p(sb_d), xo.ptr, to.ptr, C.byref(d), env.stream()) == R.WDNO_EINVAL
        x, src = Operand(n, i['x']), Operand(n, i['x0'])
        assert env.lib.wdno_apply_cond(x.ptr, src.ptr, C.byref(d), env.stream()) == R.WDNO_EINVAL
        torch.cuda.synchronize()
        xo.check('refused q_sample x', written=False)
        to.check('refused q_sample target', written=False)
        x.check('refused apply_cond x')
        assert env.K.cond_plan(d)['rc'] == R.WDNO_EINVAL


# ------------------------------------------------------------------------------------------------------------------ weighted MSE
def _run_loss(env, c, i, arm, mis, expect, gscale=None, ws_short=0):
    """arm 'fwd' | 'fwd_grad' | 'bwd' -> (loss or None, grad or None, rc)"""
    n = c['B'] * c['per_sample']
    out, tgt = Operand(n, i['out'], mis == 'out'), Operand(n, i['tgt'], mis == 'tgt')
    grad = Operand(n, misalign=mis == 'grad') if arm != 'fwd' else None
    wc, wb = _dev(i['wc']), _dev(i['wb'])
    arg = (c['B'], c['per_sample'], c['C'], c['inner'])
    if arm == 'bwd':
        p = env.K.weighted_mse_plan(*arg, backward=True, align_mask=_mask(out, tgt, grad))
        assert p['rc'] == 0 and R.plan_tuple(p) == expect, p
        g = None if gscale is None else _dev(np.asarray([gscale], np.float32))
        rc = env.lib.wdno_weighted_mse_bwd(out.ptr, tgt.ptr, env.p(wc), env.p(wb), float(i['inv']), env.p(g), grad.ptr, *arg, env.stream())
        assert rc == 0
        loss = None
    else:
        nb = env.lib.wdno_weighted_mse_ws_bytes(n) // 8
        ws = Operand(nb, dtype=torch.float64)
        loss = Operand(1)
        ws_bytes = nb * 8 - ws_short
        p = env.K.weighted_mse_plan(*arg, ws_bytes=ws_bytes, align_mask=_mask(out, tgt, grad))
        rc = env.lib.wdno_weighted_mse(out.ptr, tgt.ptr, env.p(wc), env.p(wb), float(i['inv']), loss.ptr, _ptr(grad), *arg, ws.ptr, ws_bytes, env.stream())
        assert rc == p['rc']
        if ws_short:
            torch.cuda.synchronize()
            loss.check('refused loss', written=False)
            ws.check('refused workspace', written=False)
            if grad is not None:
                grad.check('refused grad', written=False)
            return None, None, rc
        assert rc == 0 and R.plan_tuple(p) == expect, p
        ws.check('workspace')
        loss.check('loss')
    out.check('out')
    tgt.check('tgt')
    if grad is not None:
        grad.check('grad')
    shape = (c['B'], c['F'], c['C'], c['inner'])
    return (None if loss is None else loss.numpy((1,))), (None if grad is None else grad.numpy(shape)), 0


@pytest.mark.parametrize('name', list(R.LOSS_BY_NAME))
def test_loss_gate(env, name):
    c = R.LOSS_BY_NAME[name]
    K = env.K
    i = R.loss_inputs(c)
    dims = (c['F'], c['C'], c['inner'])
    base = (i['out'], i['tgt'], i['wc'], i['wb'], i['inv'])
    mis = c['misalign']
    for arm, p in R.loss_plans(K, c).items():
        assert p['rc'] == 0 and R.plan_tuple(p) == R.loss_expect(c, arm), (arm, p)
    ref_loss, s_loss = float(R.loss_value(R.F64, *base, *dims)), R.loss_scale(*base, *dims)
    mis_fwd = None if mis == 'grad' else mis
    l1, _, _ = _run_loss(env, c, i, 'fwd', mis_fwd, R.loss_expect(c, 'fwd'))
    l2, _, _ = _run_loss(env, c, i, 'fwd', mis_fwd, R.loss_expect(c, 'fwd'))
    l3, g1, _ = _run_loss(env, c, i, 'fwd_grad', mis, c['fwd'])
    l4, g2, _ = _run_loss(env, c, i, 'fwd_grad', mis, c['fwd'])
    assert _same(l1, l2) and _same(l3, l4) and _same(g1, g2), 'second run'
    if R.loss_expect(c, 'fwd') == c['fwd']:
        assert _same(l1, l3), 'the loss with and without the fused gradient'
    for got in (l1, l3):
        r = abs(float(got[0]) - ref_loss) / (R.U * s_loss)
        _report('loss', c['fwd'][0] if got is l3 else R.loss_expect(c, 'fwd')[0], 'loss', r, R.K_LOSS, name)
        assert r <= R.K_LOSS, r
    r = R.ratio(g1, R.loss_grad(R.F64, *base, *dims, fused_arm=True), R.loss_grad_scale(*base, *dims))
    _report('loss', c['fwd'][0], 'fused-grad', r, R.K_GRAD, name)
    assert r <= R.K_GRAD, r
    grads = {}
    for gscale in (None, i['gscale']):
        b1 = _run_loss(env, c, i, 'bwd', mis, c['bwd'], gscale)[1]
        assert _same(b1, _run_loss(env, c, i, 'bwd', mis, c['bwd'], gscale)[1]), 'second run'
        r = R.ratio(b1, R.loss_grad(R.F64, *base, *dims, gscale=gscale), R.loss_grad_scale(*base, *dims, gscale=gscale))
        _report('loss', c['bwd'][0], 'bwd-gscale' if gscale is not None else 'bwd', r, R.K_BWD, name)
        assert r <= R.K_BWD, r
        grads[gscale is not None] = b1
    if mis:                                                                                # the same bits whatever the alignment
        f4 = R.LOSS_BY_NAME['float4']
        _, ga, _ = _run_loss(env, c, i, 'fwd_grad', None, f4['fwd'])
        ba = _run_loss(env, c, i, 'bwd', None, f4['bwd'], i['gscale'])[1]
        assert _same(g1, ga) and _same(grads[True], ba), 'scalar against float4'
        print(f'PIN loss {name}: scalar == float4 (gradients)')
    elif not name.startswith('rounds'):                                                    # the wrapper and its autograd
        o = _dev(i['out']).requires_grad_(True)
        lw = K.weighted_mse(o, _dev(i['tgt']), _dev(i['wc']), _dev(i['wb']), c['C'], c['inner'])
        lw.backward()
        assert _same(lw.detach().cpu().numpy().reshape(1), l1) and _same(o.grad.cpu().numpy(), grads[False]), 'wrapper'


def test_loss_workspace_too_small(env):
    """one byte short of wdno_weighted_mse_ws_bytes: WDNO_EWORKSPACE from the plan and the launch, nothing written"""
    for name in ('float4', 'scalar-inner'):
        c = R.LOSS_BY_NAME[name]
        i = R.loss_inputs(c)
        for arm in ('fwd', 'fwd_grad'):
            assert _run_loss(env, c, i, arm, None, None, ws_short=1)[2] == R.WDNO_EWORKSPACE


# ------------------------------------------------------------------------------------------------------------------ sampler updates
def _run_update(env, c, i, arm, mis, tabs_d, coef, coef_d):
    """one launch of an arm of R.UPDATE_ARMS -> (x_next, x_start or None)"""
    fam, operands, kind = R.UPDATE_ARMS[arm]
    n = c['B'] * c['per_sample']
    x, eps = Operand(n, i['x'], mis == 'x'), Operand(n, i['eps'], mis == 'eps')
    nz = Operand(n, i['noise'], mis == 'noise') if 'noise' in operands else None
    xn = Operand(n, misalign=mis == 'x_next')
    xs = Operand(n, misalign=mis == 'x_start') if 'x_start' in operands else None
    p = env.K.update_plan(c['B'], c['per_sample'], _mask(x, eps, nz, xn, xs))
    expect = R.update_expect(c, operands) if mis == c['misalign'] else R.UPDATE_BY_NAME['float4']['expect']      # (the aligned re-run of an offset case)
    assert p['rc'] == 0 and R.plan_tuple(p) == expect, (arm, p)
    t = _dev(i['t'])
    tp = [env.p(v) for v in tabs_d]
    if fam == 'p_sample':
        rc = env.lib.wdno_p_sample_update(x.ptr, eps.ptr, _ptr(nz), env.p(t), *tp, xn.ptr, _ptr(xs), c['B'], c['per_sample'], int(kind != 'clamp-off'),
                                          env.stream())
    elif kind == 'dev':
        rc = env.lib.wdno_ddim_update_dev(x.ptr, eps.ptr, nz.ptr, env.p(t), tp[0], tp[1], env.p(coef_d), xn.ptr, xs.ptr, c['B'], c['per_sample'], env.stream())
    else:
        rc = env.lib.wdno_ddim_update(x.ptr, eps.ptr, _ptr(nz), env.p(t), tp[0], tp[1], *coef, xn.ptr, _ptr(xs), c['B'], c['per_sample'], env.stream())
    assert rc == 0
    for o, w in ((x, 'x'), (eps, 'eps'), (nz, 'noise'), (xn, 'x_next'), (xs, 'x_start')):
        if o is not None:
            o.check(f'{arm} {w}')
    shape = (c['B'], c['per_sample'])
    return xn.numpy(shape), (None if xs is None else xs.numpy(shape))


@pytest.mark.parametrize('name', list(R.UPDATE_BY_NAME))
def test_update_gate(env, name):
    c = R.UPDATE_BY_NAME[name]
    K = env.K
    i = R.update_inputs(c)
    tab, coef = R.update_tables(), R.ddim_coef()
    tabs_d = [_dev(v) for v in tab]
    coef_d = _dev(np.asarray(coef, np.float32))
    mis = c['misalign']
    got = {}
    for arm, (fam, operands, kind) in R.UPDATE_ARMS.items():
        noise = i['noise'] if 'noise' in operands else None
        n1, s1 = _run_update(env, c, i, arm, mis, tabs_d, coef, coef_d)
        n2, s2 = _run_update(env, c, i, arm, mis, tabs_d, coef, coef_d)
        assert _same(n1, n2) and (s1 is None or _same(s1, s2)), (arm, 'second run')
        got[arm] = (n1, s1)
        form = R.update_expect(c, operands)[0]
        if fam == 'p_sample':
            clamp = kind != 'clamp-off'
            ref_n, ref_s = R.ddpm_update(R.F64, i['x'], i['eps'], noise, i['t'], tab, clamp)
            s_n, s_s = R.ddpm_scale(i['x'], i['eps'], noise, i['t'], tab, clamp)
            k = R.K_DDPM if noise is None else R.K_DDPM_NOISE
        else:
            clamp = True
            ref_n, ref_s = R.ddim_update(R.F64, i['x'], i['eps'], noise, i['t'], tab, coef)
            s_n, s_s = R.ddim_scale(i['x'], i['eps'], noise, i['t'], tab, coef)
            k = R.K_DDIM if noise is not None else R.K_XS
        r = R.ratio(n1, ref_n, s_n)
        _report(fam, form, f'x_next[{kind}]', r, k, name)
        assert r <= k, (arm, r)
        if s1 is not None:
            r = R.ratio(s1, ref_s, s_s)
            _report(fam, form, f'x_start[{kind}]', r, R.K_XS, name)
            assert r <= R.K_XS, (arm, r)
            if clamp:
                assert np.abs(s1).max() <= 1.0 and (s1 == 1.0).any() and (s1 == -1.0).any(), (arm, 'clamped x_start lies in [-1, 1]')
            else:
                assert np.abs(s1).max() > 1.0
    assert _same(got['ddim-dev'][0], got['ddim'][0]) and _same(got['ddim-dev'][1], got['ddim'][1]), 'DDIM-dev == DDIM'
    assert _same(got['ddpm-no-x_start'][0], got['ddpm'][0]) and _same(got['ddim-no-x_start'][0], got['ddim'][0]), 'x_next with and without x_start'
    assert _same(got['ddim-no-noise'][0], got['ddim'][1]), 'the last DDIM step returns x_start'
    if mis:                                                                                # the same bits whatever the alignment
        for arm in ('ddpm', 'ddim', 'ddim-dev'):
            na, sa = _run_update(env, c, i, arm, None, tabs_d, coef, coef_d)
            assert _same(na, got[arm][0]) and _same(sa, got[arm][1]), (arm, 'scalar against float4')
        print(f'PIN update {name}: scalar == float4')
    elif not name.startswith('rounds') and c['B'] < 1000:                                  # the wrappers
        mod = types.SimpleNamespace(sqrt_recip_alphas_cumprod=tabs_d[0], sqrt_recipm1_alphas_cumprod=tabs_d[1], posterior_mean_coef1=tabs_d[2],
                                    posterior_mean_coef2=tabs_d[3], posterior_log_variance_clipped=tabs_d[4])
        x, eps, nz, t = _dev(i['x']), _dev(i['eps']), _dev(i['noise']), _dev(i['t'])
        for arm, res in (('ddpm', K.p_sample_update(mod, x, eps, nz, t, clamp=True)), ('ddpm-no-noise', K.p_sample_update(mod, x, eps, None, t, clamp=True)),
                         ('ddpm-clamp-off', K.p_sample_update(mod, x, eps, nz, t, clamp=False)), ('ddim', K.ddim_update(mod, x, eps, nz, t, *coef)),
                         ('ddim-no-noise', K.ddim_update(mod, x, eps, None, t, 0., 0., 0.)), ('ddim-dev', K.ddim_update_dev(mod, x, eps, nz, t, coef_d))):
            assert _same(res[0].cpu().numpy(), got[arm][0]) and _same(res[1].cpu().numpy(), got[arm][1]), (arm, 'wrapper')


def test_coverage(env):
    """the plans of the matrix reach every kernel of the unit in every arm; a change of the dispatch has to revisit the matrix instead of
    silently emptying a regime"""
    print(R.check_coverage(env.K))
