"""The fused attention kernels (csrc/attn_fused*.hip, csrc/linattn_fused*.hip) held ELEMENT BY ELEMENT to the fp64 references of
tests/attn_ref.py, |got - ref| <= K 2^-24 scale + flush, on a case matrix that visits every launch regime (grid-stride walk with and without
carry, HW = 1, nseq == grid, minimum / one-token / empty / capped token chunks, several items per block) and the input and gradient families
that drive the running plane scales and the online softmax. K comes from the CPU transcription (tests/test_host_attn_ref.py), not from the
kernels. Every case asserts from the library's plan queries that it reaches the regime it exists for. Also here: exact amax records,
bit-reproducibility, results that do not depend on which block or pass handled a sequence / frame, and equal bits under the bf16 mode of the
convolutions. The kernels are reached through the model's modules, the way production reaches them."""
import sys

import pytest
import torch

from tests import attn_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def mods():
    from wdno_amd import ops, tree_path
    for t in ('third_party', 'smoke', 'burgers'):
        p = tree_path(t)
        if p not in sys.path:
            sys.path.insert(0, p)
    from video_diffusion_pytorch import video_diffusion_pytorch_conv3d as V
    return ops, V


def _t_block(V, t):
    """Residual(PreNorm(temporal attention)) and the relative-position module with the parameters of t = R.t_inputs(...), on the device."""
    c = t['x'].shape[-1]
    rot = None
    if t['freqs'] is not None:
        rot = V.RotaryEmbedding(32)
        assert torch.equal(rot.freqs.data, t['freqs'])
    att = V.Attention(c, heads=4, dim_head=32, rotary_emb=rot)
    blk = V.Residual(V.PreNorm(c, V.EinopsToAndFrom('b c f h w', 'b (h w) f c', att)))
    rpb = V.RelativePositionBias(heads=4, max_distance=32) if t['emb'] is not None else None
    with torch.no_grad():
        blk.fn.norm.gamma.copy_(t['gamma'].reshape(1, c, 1, 1, 1))
        att.to_qkv.weight.copy_(t['wq'])
        att.to_out.weight.copy_(t['wo'])
        if rpb is not None:
            rpb.relative_attention_bias.weight.copy_(t['emb'])
    return blk.to(DEV), att, (rpb.to(DEV) if rpb is not None else None)


def _l_block(V, t):
    c = t['x'].shape[-1]
    blk = V.Residual(V.PreNorm(c, V.SpatialLinearAttention(c, heads=4)))
    with torch.no_grad():
        blk.fn.norm.gamma.copy_(t['gamma'].reshape(1, c, 1, 1, 1))
        blk.fn.fn.to_qkv.weight.copy_(t['wq'].reshape(384, c, 1, 1))
        blk.fn.fn.to_out.weight.copy_(t['wo'].reshape(c, 128, 1, 1))
        blk.fn.fn.to_out.bias.copy_(t['bo'])
    return blk.to(DEV)


def _run(ops, call, x, dy, params, dy_record=False):
    """One pass of call(x) through the product path: {name: tensor}, the kernels seen, the amax record dx arrived with. dy None: under
    no_grad. dy_record: dy reaches the backward as a tensor with a known amax record (as a producer kernel leaves it), else as a fresh one."""
    out, seen = {}, {}
    ops.PROFILE = {}
    try:
        if dy is None:
            with torch.no_grad():
                y = call(x)
        else:
            for p_ in params.values():
                p_.grad = None
            xr = x.detach().clone().requires_grad_(True)
            xr.register_hook(lambda g: seen.__setitem__('rec', ops._known_amax(g)))
            y = call(xr)
            g = dy.clone()
            if dy_record:
                ops._leave_amax(g, ops.tensor_amax(g))
            y.backward(g)
            out['dx'] = xr.grad.clone()
            out.update({k: p_.grad.clone() for k, p_ in params.items()})
            if 'bias' in getattr(call, 'holder', {}):
                out['dbias'] = call.holder.pop('bias').grad.clone()
        used = set(ops.PROFILE)
    finally:
        ops.PROFILE = None
    out['y'] = y.detach()
    return out, used, seen.get('rec'), ops._known_amax(y)


def _gate(got, ref, x, dy, kind_of, label):
    """Every output of `got` (device tensors) against the gate; prints ratio / K per output."""
    vals = {k: v.double().cpu() for k, v in got.items()}
    vals['branch'] = vals['y'] - x.double()
    if 'dx' in vals:
        vals['dx_branch'] = vals['dx'] - dy.double()
    rs = R.ratios({k: v.reshape(ref[0][k].shape) for k, v in vals.items()}, ref)
    assert set(rs) == set(ref[0]), (set(rs), set(ref[0]))
    rel = {k: r / R.K[kind_of(k)] for k, r in rs.items()}
    print(f'{label}: ratio / K  ' + '  '.join(f'{k} {v:.3f}' for k, v in rel.items()))
    assert all(torch.isfinite(v).all() for v in vals.values())
    bad = {k: v for k, v in rel.items() if not v <= 1.0}
    assert not bad, bad
    return rel


def _t_call(blk, rpb, f):
    """x -> block(x); the bias tensor of the last call stays in call.holder so that its gradient (dbias) can be read."""
    def call(x_):
        bias = None if rpb is None else rpb(f, device=DEV)
        if bias is not None and bias.requires_grad:
            bias.retain_grad()
            call.holder['bias'] = bias
        return blk(x_, pos_bias=bias)
    call.holder = {}
    return call


def _t_params(blk, att, rpb):
    p = {'dgamma': blk.fn.norm.gamma, 'dwq': att.to_qkv.weight, 'dwo': att.to_out.weight}
    if rpb is not None:
        p['demb'] = rpb.relative_attention_bias.weight
    return p


# ------------------------------------------------------------------------------------------------------------------ regimes
@pytest.mark.parametrize('case', sorted({e[0] for e in R.T_MATRIX}), ids=str)
def test_case_reaches_its_regime_temporal(mods, case):
    ops, _ = mods
    c, b, f, h, w = case
    x = torch.empty(b, f, h, w, c, device=DEV)
    with torch.no_grad():
        assert ops.tattn_fused_takes(x, 4, ())
    if c == 64 and f == 24:
        assert ops.tattn_fused_takes(x.requires_grad_(True), 4, ())
    plan = ops.tattn_fused_plan(c, f, b, h * w)
    want = R.t_regime(case)
    assert {k: plan.get(k) for k in want} == want, plan


@pytest.mark.parametrize('case', sorted({e[0] for e in R.L_MATRIX}), ids=str)
def test_case_reaches_its_regime_linear(mods, case):
    ops, _ = mods
    c, b, f, h, w = case
    x = torch.empty(b, f, h, w, c, device=DEV)
    with torch.no_grad():
        assert ops.lattn_fused_takes(x, 4, ())
    if c == 64:
        assert ops.lattn_fused_takes(x.requires_grad_(True), 4, ())
    plan = R.l_plan_view(ops.lattn_fused_plan(b * f, h * w), h * w)
    plan['items_per_block'] = -(-b * f * plan['chunks2'] // plan['grid2'])
    want = R.l_regime(case)
    assert {k: plan.get(k) for k in want} == want, plan


# ------------------------------------------------------------------------------------------------------------------ element-wise gates
@pytest.mark.parametrize('entry', R.T_MATRIX, ids=R.case_id)
def test_temporal_gate(mods, entry):
    ops, V = mods
    case, family, grad, rot_bias = entry
    t = R.t_inputs(*entry)
    ref = R.reference_of_t(entry)
    blk, att, rpb = _t_block(V, t)
    x = t['x'].to(DEV)
    dy = t['dy'].to(DEV) if grad is not None else None
    call, params = _t_call(blk, rpb, case[2]), _t_params(blk, att, rpb)
    got, used, rec_dx, rec_y = _run(ops, call, x, dy, params)
    assert 'tattn_fused_fwd_kernel' in used and (grad is None) == ('tattn_fused_bwd_kernel' not in used), used
    assert not any('conv' in k or 'layernorm' in k or 'attn_bwd' in k for k in used), used
    _gate(got, ref, t['x'], t.get('dy'), R.kind_t, R.case_id(entry))
    # amax records are exact; a second run returns the same bits
    assert rec_y is not None and rec_y.max().item() == got['y'].abs().max().item()
    got2, _, _, _ = _run(ops, call, x, dy, params, dy_record=True)
    if grad is not None:
        assert rec_dx is not None and rec_dx.max().item() == got['dx'].abs().max().item()
        _gate(got2, ref, t['x'], t['dy'], R.kind_t, R.case_id(entry) + ' (dy with a record)')
    assert all(torch.equal(got[k], got2[k]) for k in got)
    if grad == 'zero':
        assert torch.equal(got['dx'], dy) and all(not got[k].any() for k in params)


@pytest.mark.parametrize('entry', R.L_MATRIX, ids=R.case_id)
def test_linear_gate(mods, entry):
    ops, V = mods
    case, family, grad = entry
    n_tok = case[3] * case[4]
    t = R.l_inputs(*entry)
    ref = R.reference_of_l(entry)
    blk = _l_block(V, t)
    x = t['x'].to(DEV)
    dy = t['dy'].to(DEV) if grad is not None else None
    params = {'dgamma': blk.fn.norm.gamma, 'dwq': blk.fn.fn.to_qkv.weight, 'dwo': blk.fn.fn.to_out.weight, 'db_out': blk.fn.fn.to_out.bias}
    got, used, rec_dx, rec_y = _run(ops, blk, x, dy, params)
    assert 'lattn_fused_fwd_kernels' in used and (grad is None) == ('lattn_fused_bwd_kernels' not in used), used
    assert not any('conv' in k or 'layernorm' in k or 'linattn' in k for k in used), used
    kind = lambda k: R.kind_l(k, n_tok)
    _gate(got, ref, t['x'], t.get('dy'), kind, R.case_id(entry))
    assert rec_y is not None and rec_y.max().item() == got['y'].abs().max().item()
    got2, _, _, _ = _run(ops, blk, x, dy, params, dy_record=True)
    if grad is not None:
        assert rec_dx is not None and rec_dx.max().item() == got['dx'].abs().max().item()
        _gate(got2, ref, t['x'], t['dy'], kind, R.case_id(entry) + ' (dy with a record)')
    assert all(torch.equal(got[k], got2[k]) for k in got)
    if grad == 'zero':
        assert torch.equal(got['dx'], dy) and all(not got[k].any() for k in params)


# ------------------------------------------------------------------------------------------------------------------ placement invariance
@pytest.mark.parametrize('c,f', [(64, 24), (64, 48), (128, 24), (256, 24)])
def test_a_sequence_does_not_depend_on_the_block_or_pass_that_handled_it(mods, c, f):
    """The samples of the 9-sample case (two or three passes, carry) run alone (77 sequences, one pass, one block each): the same bits."""
    ops, V = mods
    case = R.t_case(c, f, 'carry')
    t = R.t_inputs(case, 'gauss', None, True)
    blk, att, rpb = _t_block(V, t)
    call = _t_call(blk, rpb, f)
    x = t['x'].to(DEV)
    plan9, plan1 = ops.tattn_fused_plan(c, f, 9, 77), ops.tattn_fused_plan(c, f, 1, 77)
    assert plan9['passes_fwd'] > 1 and plan1['passes_fwd'] == 1 and plan1['grid_fwd'] == 77
    with torch.no_grad():
        y9 = call(x)
        for j in (0, 4, 8):
            xj = x[j:j + 1].contiguous()
            assert ops.tattn_fused_takes(xj, 4, ())
            assert torch.equal(call(xj)[0], y9[j]), j


def test_a_frame_does_not_depend_on_its_position_in_the_batch(mods):
    """Linear attention: the frames of a case in another order (the same number of units: the same cut into chunks) give the same rows."""
    ops, V = mods
    for name in ('empty', 'one_token'):
        case = R.l_case(64, name)
        t = R.l_inputs(case, 'gauss', None)
        blk = _l_block(V, t)
        x = t['x'].to(DEV)
        f = x.shape[1]
        perm = torch.roll(torch.arange(f), 1)
        assert ops.lattn_fused_plan(f, case[3] * case[4]) == ops.lattn_fused_plan(x[:, perm].shape[1], case[3] * case[4])
        with torch.no_grad():
            assert torch.equal(blk(x)[:, perm], blk(x[:, perm].contiguous()))


# ------------------------------------------------------------------------------------------------------------------ mode equality
@pytest.mark.parametrize('family', ['temporal', 'temporal48', 'temporal_wide', 'linear', 'linear_wide'])
def test_bf16_mode_of_the_convolutions_does_not_change_the_fused_blocks(mods, family):
    """ops._in_f16x3: the fused blocks compute on the split-fp16 planes whatever ops.CONV_MATH is -- equal bits, forward and backward."""
    ops, V = mods
    if family.startswith('temporal'):
        c, f = {'temporal': (64, 24), 'temporal48': (64, 48), 'temporal_wide': (128, 24)}[family]
        grad = 'gauss' if family == 'temporal' else None
        t = R.t_inputs(R.t_case(c, f, 'min'), 'gauss', grad, True)
        blk, att, rpb = _t_block(V, t)
        call, params = _t_call(blk, rpb, f), _t_params(blk, att, rpb)
        kernels = {'tattn_fused_fwd_kernel'} | ({'tattn_fused_bwd_kernel'} if grad else set())
    else:
        c = 64 if family == 'linear' else 128
        grad = 'gauss' if family == 'linear' else None
        t = R.l_inputs(R.l_case(c, 'one_token'), 'gauss', grad)
        blk = _l_block(V, t)
        call = blk
        params = {'dgamma': blk.fn.norm.gamma, 'dwq': blk.fn.fn.to_qkv.weight, 'dwo': blk.fn.fn.to_out.weight, 'db_out': blk.fn.fn.to_out.bias}
        kernels = {'lattn_fused_fwd_kernels'} | ({'lattn_fused_bwd_kernels'} if grad else set())
    x = t['x'].to(DEV)
    dy = t['dy'].to(DEV) if grad else None
    got, used, _, _ = _run(ops, call, x, dy, params)
    assert kernels <= used, used
    prev = ops.CONV_MATH
    ops.CONV_MATH = 'bf16'
    try:
        got_b, used_b, _, _ = _run(ops, call, x, dy, params)
    finally:
        ops.CONV_MATH = prev
    assert kernels <= used_b, used_b
    assert set(got) == set(got_b) and all(torch.equal(got[k], got_b[k]) for k in got)
