"""tests/attn_ref.py against the oracle itself (no GPU): the fp64 references agree with oracle/unet_ref.py's channel_layernorm + token_attention /
linear_attention_2d and the hand-written backwards with their autograd, every scale bounds its value, the fp32 transcription of the kernels'
arithmetic stays within HALF of every gate on the whole case matrix (so K is the reference's own error and four-fold room for the device, not
a fit to the kernels), K is pinned to the measurement from both sides, and every case reaches the regime it exists for as far as the library
answers that without a device (wdno_num_cus() falls back to 256 compute units there)."""
import functools

import pytest

from oracle import unet_ref as O
from tests import attn_ref as R


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _oracle_t(t):
    """(y, {name: gradient}) of the temporal block by the oracle's functions and autograd, fp64 (eps: the C float the library receives)."""
    leaf = {k: v.detach().double().requires_grad_(True) for k, v in t.items() if v is not None and k not in ('freqs', 'dy')}
    xc = leaf['x'].permute(0, 4, 1, 2, 3)
    f = xc.shape[2]
    bias = O.time_rel_pos_bias(leaf['emb'], f) if 'emb' in leaf else None
    y = O.channel_layernorm(xc, leaf['gamma'].reshape(1, -1, 1, 1, 1), eps=R.EPS)
    b, c, f, h, w = y.shape
    y = O.token_attention(y.permute(0, 3, 4, 2, 1).reshape(b, h * w, f, c), leaf['wq'], leaf['wo'], 4, 32,
                          freqs=None if t['freqs'] is None else t['freqs'].double(), pos_bias=bias)
    y = (y.reshape(b, h, w, f, c).permute(0, 4, 3, 1, 2) + xc).permute(0, 2, 3, 4, 1)
    if t.get('dy') is not None:
        y.backward(t['dy'].double())
    return y.detach(), {k: v.grad for k, v in leaf.items()}


def _oracle_l(t):
    leaf = {k: v.detach().double().requires_grad_(True) for k, v in t.items() if v is not None and k != 'dy'}
    xc = leaf['x'].permute(0, 4, 1, 2, 3)
    y = O.channel_layernorm(xc, leaf['gamma'].reshape(1, -1, 1, 1, 1), eps=R.EPS)
    b, c, f, h, w = y.shape
    y = O.linear_attention_2d(y.permute(0, 2, 1, 3, 4).reshape(b * f, c, h, w), leaf['wq'][:, :, None, None], leaf['wo'][:, :, None, None], leaf['bo'], 4, 32)
    y = (y.reshape(b, f, c, h, w).permute(0, 2, 1, 3, 4) + xc).permute(0, 2, 3, 4, 1)
    if t.get('dy') is not None:
        y.backward(t['dy'].double())
    return y.detach(), {k: v.grad for k, v in leaf.items()}


T_ORACLE = [((64, 3, 24, 7, 11), 'gauss', 'gauss', True), ((64, 1, 24, 8, 8), 'const', 'gauss', True), ((64, 1, 24, 8, 8), 'gauss', 'ramp_up', False),
            ((64, 1, 24, 8, 8), 'sharp', 'holes', True), ((64, 1, 48, 8, 8), 'offset', None, True), ((128, 1, 24, 8, 8), 'gauss', None, True),
            ((256, 1, 24, 8, 8), 'gauss', None, False)]
L_ORACLE = [((64, 2, 3, 7, 11), 'gauss', 'gauss'), ((64, 1, 2, 3, 11), 'k_up', 'gauss'), ((64, 1, 5, 20, 20), 'const', 'gauss'),
            ((64, 1, 2, 4, 8), 'sharp', 'ramp_down'), ((64, 1, 2, 4, 8), 'offset', 'gauss'), ((128, 1, 2, 4, 8), 'gauss', None), ((256, 1, 2, 3, 11), 'k_down', None)]
_NAMES_T = {'dx': 'x', 'dgamma': 'gamma', 'dwq': 'wq', 'dwo': 'wo', 'demb': 'emb'}
_NAMES_L = {'dx': 'x', 'dgamma': 'gamma', 'dwq': 'wq', 'dwo': 'wo', 'db_out': 'bo'}


@pytest.mark.parametrize('entry', T_ORACLE, ids=R.case_id)
def test_temporal_reference_is_the_oracle_and_its_autograd(entry):
    t = R.t_inputs(*entry)
    out, scale, flush, _ = R.reference_of_t(entry)
    y, grads = _oracle_t(t)
    assert _rel(out['y'], y) <= 1e-12 and _rel(out['branch'], y - t['x'].double()) <= 1e-11
    for name, leaf in _NAMES_T.items():
        if name in out:
            assert _rel(out[name].reshape(grads[leaf].shape), grads[leaf]) <= 1e-12, name
    if 'dx' in out:
        assert _rel(out['dx_branch'], grads['x'] - t['dy'].double()) <= 1e-11
    for name in out:                                                     # every scale bounds its value
        assert (scale[name] >= out[name].abs() * (1 - 1e-12)).all() and (flush[name] >= 0).all(), name


@pytest.mark.parametrize('entry', L_ORACLE, ids=R.case_id)
def test_linear_reference_is_the_oracle_and_its_autograd(entry):
    t = R.l_inputs(*entry)
    out, scale, flush, _ = R.reference_of_l(entry)
    y, grads = _oracle_l(t)
    assert _rel(out['y'], y) <= 1e-12 and _rel(out['branch'], y - t['x'].double()) <= 1e-11
    for name, leaf in _NAMES_L.items():
        if name in out:
            assert _rel(out[name].reshape(grads[leaf].shape), grads[leaf]) <= 1e-12, name
    for name in out:
        assert (scale[name] >= out[name].abs() * (1 - 1e-12)).all() and (flush[name] >= 0).all(), name


def _plan_l(case):
    from wdno_amd import ops
    c, b, f, h, w = case
    return ops.lattn_fused_plan(b * f, h * w)


@functools.lru_cache(maxsize=None)
def _worst_t(entry):
    t = R.t_inputs(*entry)
    got = R.transcription_t(t['x'], t['gamma'], t['wq'], t['wo'], t['freqs'], t['emb'], t.get('dy'))
    worst = {}
    for name, r in R.ratios(got, R.reference_of_t(entry)).items():
        worst[R.kind_t(name)] = max(worst.get(R.kind_t(name), 0.0), r)
    return worst


@functools.lru_cache(maxsize=None)
def _worst_l(entry):
    t = R.l_inputs(*entry)
    n_tok = entry[0][3] * entry[0][4]
    got = R.transcription_l(t['x'], t['gamma'], t['wq'], t['wo'], t['bo'], t.get('dy'), plan=_plan_l(entry[0]))
    worst = {}
    for name, r in R.ratios(got, R.reference_of_l(entry)).items():
        k = R.kind_l(name, n_tok)
        worst[k] = max(worst.get(k, 0.0), r)
    return worst


@pytest.mark.parametrize('entry', R.T_MATRIX, ids=R.case_id)
def test_temporal_transcription_stays_within_half_the_gate(entry):
    worst = _worst_t(entry)
    print('transcription ratios', R.case_id(entry), {k: round(v, 3) for k, v in worst.items()})
    for kind, r in worst.items():
        assert r <= R.K[kind] / 2, (kind, r, R.K[kind])
    if entry[2] == 'zero':                                               # dy = 0: every gradient exactly zero, dx == dy bit for bit
        t = R.t_inputs(*entry)
        got = R.transcription_t(t['x'], t['gamma'], t['wq'], t['wo'], t['freqs'], t['emb'], t['dy'])
        assert all(not got[k].any() for k in ('dx', 'dwq', 'dwo', 'dgamma', 'dbias'))


@pytest.mark.parametrize('entry', R.L_MATRIX, ids=R.case_id)
def test_linear_transcription_stays_within_half_the_gate(entry):
    worst = _worst_l(entry)
    print('transcription ratios', R.case_id(entry), {k: round(v, 3) for k, v in worst.items()})
    for kind, r in worst.items():
        assert r <= R.K[kind] / 2, (kind, r, R.K[kind])


def test_k_is_four_times_the_measured_ratio_and_documented():
    """K = ceil(4 x the transcription's worst ratio over the whole matrix), pinned from both sides, so that a later edit of K, of the scales
    or of the matrix cannot drift the gate upwards unnoticed. (0.05 of room: the host's expf may differ by an ulp between machines.)"""
    worst = {}
    for w in [_worst_t(e) for e in R.T_MATRIX] + [_worst_l(e) for e in R.L_MATRIX]:
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print('worst transcription ratios', {k: round(v, 3) for k, v in sorted(worst.items())})
    assert set(worst) == set(R.K)
    for kind, k in R.K.items():
        assert isinstance(k, int) and k > 0
        assert k / 4 - 0.25 - 0.05 <= worst[kind] <= k / 4 + 0.05, (kind, k, worst[kind])
        assert f'{kind}: {k}' in R.__doc__, kind


def test_the_gate_sees_one_wrong_row():
    """The class of defect a whole-tensor norm cannot see: one row of y (64 of 1 064 448 values) off by 1e-3 relative moves rel-L2 by 8e-6 and the
    gate by far more than K."""
    entry = R.T_MATRIX[2]
    out, scale, flush, _ = R.reference_of_t(entry)
    got = out['y'].clone()
    got[-1, 3, 2, 5] *= 1 + 1e-3
    assert float((got - out['y']).norm() / out['y'].norm()) < 1e-5
    assert R.ratio(got, out['y'], scale['y'], flush['y']) > 4 * R.K['t_y']


@pytest.mark.parametrize('case', sorted({e[0] for e in R.T_MATRIX}), ids=str)
def test_temporal_case_reaches_its_regime_on_256_cus(case):
    from wdno_amd import _lib, ops
    _lib.load()
    c, b, f, h, w = case
    plan = ops.tattn_fused_plan(c, f, b, h * w)
    want = R.t_regime(case)
    assert {k: plan.get(k) for k in want} == want, plan


@pytest.mark.parametrize('case', sorted({e[0] for e in R.L_MATRIX}), ids=str)
def test_linear_case_reaches_its_regime_on_256_cus(case):
    from wdno_amd import _lib, ops
    _lib.load()
    c, b, f, h, w = case
    plan = R.l_plan_view(ops.lattn_fused_plan(b * f, h * w), h * w)
    plan['items_per_block'] = -(-b * f * plan['chunks2'] // plan['grid2'])
    want = R.l_regime(case)
    assert {k: plan.get(k) for k in want} == want, plan
