"""tests/groupnorm_ref.py against torch itself (no GPU): the fp64 reference agrees with F.group_norm and with autograd, the fp32
transcription of the kernels' formulas stays within HALF of every gate on the whole case matrix (so the gate's K is the reference's own
error and four-fold room for the device, not a fit to the kernels), and two faults a whole-tensor rel-L2 cannot see fail the gate."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import groupnorm_ref as R
from tests.helpers import rel_l2


def _args(case, variant, act, use_ss):
    t = R.inputs(case, variant)
    return (t['x'], t['gamma'], t['beta'], case[3], t['ss'] if use_ss else None, act, t['res'], t['dy'])


@functools.lru_cache(maxsize=None)
def _worst(cv):
    """{kind: worst ratio of the fp32 transcription} over the (act, scale_shift) combinations of one entry of the matrix."""
    case, variant = cv
    worst = {}
    for act, use_ss in R.configs(case):
        a = _args(case, variant, act, use_ss)
        for name, r in R.ratios(R.transcription(*a), R.reference_of(case, variant, act, use_ss)).items():
            worst[R.KIND[name]] = max(worst.get(R.KIND[name], 0.0), r)
    return worst


@pytest.mark.parametrize('cv', R.MATRIX, ids=R.case_id)
def test_transcription_stays_within_half_the_gate(cv):
    worst = _worst(cv)
    print('transcription ratios', R.case_id(cv), {k: round(v, 2) for k, v in worst.items()})
    for kind, r in worst.items():
        assert r <= R.K[kind] / 2, (kind, r, R.K[kind])


def test_k_is_four_times_the_measured_ratio_and_documented():
    """K = ceil(4 x the transcription's worst ratio over the whole matrix), pinned from both sides, so that a later edit of K, of the
    scales or of the matrix cannot drift the gate upwards unnoticed. (0.05 of room: the host's expf may differ by an ulp between machines.)"""
    assert all(isinstance(v, int) and v > 0 for v in R.K.values()) and set(R.KIND.values()) == set(R.K)
    for kind, k in R.K.items():
        w = max(_worst(cv).get(kind, 0.0) for cv in R.MATRIX)
        assert k / 4 - 0.25 - 0.05 <= w <= k / 4 + 0.05, (kind, k, w)
        assert f'{kind}: {k}' in R.__doc__, kind


@pytest.mark.parametrize('case', [(2, 300, 64, 8), (3, 130, 24, 4), (2, 97, 136, 2), (1, 1, 8, 1)], ids=str)
def test_reference_is_group_norm(case):
    t = R.inputs(case)
    out, _, _ = R.reference(t['x'], t['gamma'], t['beta'], case[3], None, act=False, eps=1e-5)
    ncl = t['x'].double().permute(0, 2, 1)
    want = F.group_norm(ncl, case[3], t['gamma'].double(), t['beta'].double(), eps=1e-5).permute(0, 2, 1)
    assert (out['y'] - want).abs().max() <= 1e-12 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize('case,act,use_ss', [((2, 300, 64, 8), True, True), ((3, 130, 24, 4), False, True), ((2, 97, 136, 2), True, False)], ids=str)
def test_reference_gradients_are_autograd(case, act, use_ss):
    t = R.inputs(case)
    n, s, c, g = case
    x, gam, bet, ss, res = (t[k].double().requires_grad_(True) for k in ('x', 'gamma', 'beta', 'ss', 'res'))
    y = F.group_norm(x.permute(0, 2, 1), g, gam, bet, eps=R.EPS).permute(0, 2, 1)
    if use_ss:
        y = y * (ss[:, None, :c] + 1) + ss[:, None, c:]
    if act:
        y = F.silu(y)
    ya = y + res
    ya.backward(t['dy'].double())
    out, _, _ = R.reference(t['x'], t['gamma'], t['beta'], g, t['ss'] if use_ss else None, act, t['res'], t['dy'])
    want = {'y': y.detach(), 'y_add': ya.detach(), 'dx': x.grad, 'dgamma': gam.grad, 'dbeta': bet.grad, 'colsum': x.grad.sum((0, 1))}
    if use_ss:
        want['dss'] = ss.grad
    assert torch.equal(res.grad, t['dy'].double())             # the residual's gradient is dy itself
    for k, w in want.items():
        assert (out[k] - w).abs().max() <= 1e-12 * max(1.0, float(w.abs().max())), k


def test_gate_sees_one_wrong_group_rstd():
    """rstd of one group of one sample wrong by a relative 3e-6: y and dx stay under the whole-tensor rel-L2 bars the suite used
    (2e-6 / 5e-6); the element-wise gate fails."""
    case = R.ANCHOR
    a = _args(case, 'std', True, True)
    ref = R.reference_of(case, 'std', True, True)
    bad = R.transcription(*a, rstd_error=(1, 3, 3e-6))
    assert rel_l2(bad['y'], ref[0]['y']) < 2e-6 and rel_l2(bad['dx'], ref[0]['dx']) < 5e-6
    r = R.ratios(bad, ref)
    assert r['y'] > R.K['y'] and r['dx'] > R.K['dx'], r
    good = R.ratios(R.transcription(*a), ref)
    assert all(good[k] <= R.K[R.KIND[k]] / 2 for k in good), good


def test_gate_sees_one_dropped_row():
    """One row of one sample left out of the sums over rows (a chunk's row guard off by one) in the largest sample of the matrix."""
    case = (1, 2048, 1024, 1)
    a = _args(case, 'std', True, True)
    ref = R.reference_of(case, 'std', True, True)
    bad = R.transcription(*a, drop_row=(0, 2047))
    r = R.ratios(bad, ref)
    assert r['y'] > R.K['y'] and r['dx'] > R.K['dx'] and r['dbeta'] > R.K['param'] and r['dgamma'] > R.K['param'] and r['dss'] > R.K['dss'], r
