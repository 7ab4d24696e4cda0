"""Anchors tests/diffusion_kernels_ref.py -- the fp64 reference, the error scale and the gate the kernels of csrc/diffusion.hip are held to in
tests/test_gpu_diffusion_matrix.py -- without a GPU. The per-element mask table equals the oracle's statement-order functions on every flag
combination of the matrix. For every case both fp32 transcriptions (every product and add rounded; product-then-add fused) stay within K: the
bound is shown to hold for a correct implementation before any kernel is held to it. Planted faults (a swapped priority of two mask rules, t
of the wrong sample, the channel index without F, a missing clamp) break the gate on the transcription: it has teeth. The plan queries need no
device: every case reaches the form and the grid it states, and the matrix as a whole reaches every kernel of the unit in every arm."""
import numpy as np
import pytest

from tests import diffusion_kernels_ref as R

ARITHS = {'rounded': R.F32, 'fused': R.F32FMA}


@pytest.fixture(scope='module')
def K():
    from wdno_amd import diffusion_core as k
    from wdno_amd import ops
    ops._lib_()
    return k


def _schedule(c):
    b = R.tables('sigmoid' if c['tree'] == 0 else 'cosine')
    return b['sqrt_alphas_cumprod'], b['sqrt_one_minus_alphas_cumprod']


# ------------------------------------------------------------------------------------------------------------------ masks
@pytest.mark.parametrize('name', [c['name'] for c in R.COND_CASES if not c['name'].startswith('rounds')])
def test_mask_table_equals_the_oracle(name):
    c = R.COND_BY_NAME[name]
    assert np.array_equal(R.cond_table(c), R.oracle_codes(c))


def test_masks_of_the_matrix_hold_every_code_and_overlap():
    """the shapes put all three codes into play, rules overlap (a later statement overrides an earlier one somewhere), and a float4 group
    straddles cW with different codes inside it"""
    c = R.COND_BY_NAME['smoke-w8-C82-pad+control+low']
    code = R.oracle_codes(c)[0]
    assert set(np.unique(code)) == {0, 1, 2}
    rules = {n: p for n, _, p in R.smoke_rules(c)}
    assert (rules['pad'] & rules['control']).any() and (rules['pad'] & rules['low']).any() and (rules['pad'] & rules['init']).any()
    assert (code[..., 4:8].min(axis=-1) != code[..., 4:8].max(axis=-1)).any()
    assert (code[2] != code[0]).any() and (code[:, :, 5] != code[:, :, 0]).any()          # the frame beyond cT, the row beyond cH
    c = R.COND_BY_NAME['burgers-w12-C17-pad+u0+uT+f+low']
    code = R.oracle_codes(c)[0]
    assert set(np.unique(code)) == {0, 1, 2}
    assert (code[..., 8:12].min(axis=-1) != code[..., 8:12].max(axis=-1)).any()
    rules = {n: p for n, _, p in R.burgers_rules(c)}
    assert (rules['u0'] & rules['uT']).any() and rules['uT'][-1, 11:].any()               # uT rows inside the padded rows


def test_flag_combinations_are_complete():
    names = set(R.COND_BY_NAME)
    assert sum(n.startswith('smoke-w8-C') for n in names) == 12 and sum(n.startswith('smoke-w6-C') for n in names) == 12
    assert sum(n.startswith('burgers-w12-C') for n in names) == 48 and sum(n.startswith('burgers-w14-C') for n in names) == 48
    assert {c['misalign'] for c in R.COND_CASES} == {None, *R.COND_OPERANDS}
    assert {c['misalign'] for c in R.LOSS_CASES} == {None, *R.LOSS_OPERANDS}
    assert {c['misalign'] for c in R.UPDATE_CASES} == {None, *R.UPDATE_OPERANDS}


# ------------------------------------------------------------------------------------------------------------------ the gate holds on the CPU
@pytest.mark.parametrize('name', list(R.COND_BY_NAME))
def test_cond_transcriptions_stay_within_the_gate(name):
    c = R.COND_BY_NAME[name]
    i = R.cond_inputs(c)
    sa, sb = _schedule(c)
    ref = R.cond_reference(c, i['x0'], i['noise'], i['t'], sa, sb)
    assert 0 in i['t'] and (R.T_STEPS - 1 in i['t'])
    for ar in ARITHS.values():
        x, tgt = R.cond_transcription(ar, c, i['x0'], i['noise'], i['t'], sa, sb)
        assert x.dtype == np.float32
        assert R.ratio(x, ref['x'], ref['x_scale']) <= R.K_Q
        assert np.array_equal(R.bits(tgt), R.bits(ref['target']))
    a = R.apply_reference(c, i['x'], i['x0'])
    assert np.array_equal(R.bits(a)[ref['code'] == 0], R.bits(i['x'])[ref['code'] == 0])


@pytest.mark.parametrize('name', list(R.LOSS_BY_NAME))
def test_loss_transcriptions_stay_within_the_gate(name):
    c = R.LOSS_BY_NAME[name]
    i = R.loss_inputs(c)
    dims = (c['F'], c['C'], c['inner'])
    assert len(set(i['wc'].tolist())) == c['C'] and len(set(i['wb'][:29].tolist())) == min(c['B'], 29) and c['F'] == 2
    ref_loss = R.loss_value(R.F64, i['out'], i['tgt'], i['wc'], i['wb'], i['inv'], *dims)
    s_loss = R.loss_scale(i['out'], i['tgt'], i['wc'], i['wb'], i['inv'], *dims)
    for ar in ARITHS.values():
        got = R.loss_value(ar, i['out'], i['tgt'], i['wc'], i['wb'], i['inv'], *dims)
        assert abs(float(got) - float(ref_loss)) <= R.K_LOSS * R.U * s_loss
        for gscale, fused_arm, k in ((None, True, R.K_GRAD), (None, False, R.K_BWD), (i['gscale'], False, R.K_BWD)):
            ref = R.loss_grad(R.F64, i['out'], i['tgt'], i['wc'], i['wb'], i['inv'], *dims, gscale=gscale, fused_arm=fused_arm)
            scale = R.loss_grad_scale(i['out'], i['tgt'], i['wc'], i['wb'], i['inv'], *dims, gscale=gscale)
            got = R.loss_grad(ar, i['out'], i['tgt'], i['wc'], i['wb'], i['inv'], *dims, gscale=gscale, fused_arm=fused_arm)
            assert got.dtype == np.float32 and R.ratio(got, ref, scale) <= k, (gscale, fused_arm)


@pytest.mark.parametrize('name', list(R.UPDATE_BY_NAME))
def test_update_transcriptions_stay_within_the_gate(name):
    c = R.UPDATE_BY_NAME[name]
    i = R.update_inputs(c)
    tab, coef = R.update_tables(), R.ddim_coef()
    assert 0 in i['t'] and (R.T_STEPS - 1 in i['t'])
    _, raw = R.x_start(R.F64, i['x'], i['eps'], i['t'], tab[0], tab[1], clamp=False)
    assert (raw < -1).any() and (raw > 1).any() and (np.abs(raw) < 1).any()               # x_start clamps on each side and stays free in between
    for ar in ARITHS.values():
        for noise, clamp in ((i['noise'], True), (None, True), (i['noise'], False)):
            ref_n, ref_s = R.ddpm_update(R.F64, i['x'], i['eps'], noise, i['t'], tab, clamp)
            s_n, s_s = R.ddpm_scale(i['x'], i['eps'], noise, i['t'], tab, clamp)
            got_n, got_s = R.ddpm_update(ar, i['x'], i['eps'], noise, i['t'], tab, clamp)
            assert got_n.dtype == np.float32
            assert R.ratio(got_s, ref_s, s_s) <= R.K_XS
            assert R.ratio(got_n, ref_n, s_n) <= (R.K_DDPM if noise is None else R.K_DDPM_NOISE - 2 * R.EXPF_ULPS)      # (exp is correctly rounded here)
        for noise in (i['noise'], None):
            ref_n, ref_s = R.ddim_update(R.F64, i['x'], i['eps'], noise, i['t'], tab, coef)
            s_n, s_s = R.ddim_scale(i['x'], i['eps'], noise, i['t'], tab, coef)
            got_n, got_s = R.ddim_update(ar, i['x'], i['eps'], noise, i['t'], tab, coef)
            assert R.ratio(got_s, ref_s, s_s) <= R.K_XS and np.abs(got_s).max() <= 1.0
            assert R.ratio(got_n, ref_n, s_n) <= (R.K_DDIM if noise is not None else R.K_XS)


# ------------------------------------------------------------------------------------------------------------------ planted faults
def test_planted_swapped_mask_priority_breaks_the_gate():
    for name, swap in (('smoke-w8-C82-pad+control+low', ('pad', 'low')), ('smoke-w8-C42-pad+control', ('control', 'pad')),
                       ('smoke-w6-C42-pad', ('init', 'pad'))):
        c = R.COND_BY_NAME[name]
        i = R.cond_inputs(c)
        sa, sb = _schedule(c)
        ref = R.cond_reference(c, i['x0'], i['noise'], i['t'], sa, sb)
        bad = R.cond_table(c, swap=swap)
        assert not np.array_equal(bad, R.oracle_codes(c))
        x, tgt = R.cond_transcription(R.F32, c, i['x0'], i['noise'], i['t'], sa, sb, code=bad)
        assert R.ratio(x, ref['x'], ref['x_scale']) > R.K_Q
        a = R.apply_reference(c, i['x'], i['x0'], code=bad)
        assert not np.array_equal(R.bits(a), R.bits(R.apply_reference(c, i['x'], i['x0'])))


def test_planted_t_of_the_wrong_sample_breaks_the_gate():
    c = R.COND_BY_NAME['burgers-w14-C9-pad+u0+uT+f']
    i = R.cond_inputs(c)
    sa, sb = _schedule(c)
    ref = R.cond_reference(c, i['x0'], i['noise'], i['t'], sa, sb)
    x, _ = R.cond_transcription(R.F32, c, i['x0'], i['noise'], i['t'], sa, sb, t_shift=1)
    assert R.ratio(x, ref['x'], ref['x_scale']) > R.K_Q
    c = R.UPDATE_BY_NAME['scalar-odd']
    i = R.update_inputs(c)
    tab, coef = R.update_tables(), R.ddim_coef()
    ref_n, ref_s = R.ddpm_update(R.F64, i['x'], i['eps'], i['noise'], i['t'], tab)
    s_n, s_s = R.ddpm_scale(i['x'], i['eps'], i['noise'], i['t'], tab)
    got_n, got_s = R.ddpm_update(R.F32, i['x'], i['eps'], i['noise'], i['t'], tab, t_shift=1)
    assert R.ratio(got_s, ref_s, s_s) > R.K_XS and R.ratio(got_n, ref_n, s_n) > R.K_DDPM_NOISE
    ref_n, ref_s = R.ddim_update(R.F64, i['x'], i['eps'], i['noise'], i['t'], tab, coef)
    s_n, s_s = R.ddim_scale(i['x'], i['eps'], i['noise'], i['t'], tab, coef)
    got_n, got_s = R.ddim_update(R.F32, i['x'], i['eps'], i['noise'], i['t'], tab, coef, t_shift=1)
    assert R.ratio(got_s, ref_s, s_s) > R.K_XS and R.ratio(got_n, ref_n, s_n) > R.K_DDIM


def test_planted_channel_index_without_f_breaks_the_gate():
    c = R.LOSS_BY_NAME['float4']
    i = R.loss_inputs(c)
    dims = (c['F'], c['C'], c['inner'])
    ref = R.loss_grad(R.F64, i['out'], i['tgt'], i['wc'], i['wb'], i['inv'], *dims)
    scale = R.loss_grad_scale(i['out'], i['tgt'], i['wc'], i['wb'], i['inv'], *dims)
    got = R.loss_grad(R.F32, i['out'], i['tgt'], i['wc'], i['wb'], i['inv'], *dims, chan_without_f=True)
    assert R.ratio(got, ref, scale) > R.K_BWD
    ref_loss = R.loss_value(R.F64, i['out'], i['tgt'], i['wc'], i['wb'], i['inv'], *dims)
    bad_loss = R.loss_value(R.F32, i['out'], i['tgt'], i['wc'], i['wb'], i['inv'], *dims, chan_without_f=True)
    assert abs(float(bad_loss) - float(ref_loss)) > R.K_LOSS * R.U * R.loss_scale(i['out'], i['tgt'], i['wc'], i['wb'], i['inv'], *dims)


def test_planted_missing_clamp_breaks_the_gate():
    c = R.UPDATE_BY_NAME['float4']
    i = R.update_inputs(c)
    tab, coef = R.update_tables(), R.ddim_coef()
    ref_n, ref_s = R.ddpm_update(R.F64, i['x'], i['eps'], i['noise'], i['t'], tab)
    s_n, s_s = R.ddpm_scale(i['x'], i['eps'], i['noise'], i['t'], tab)
    got_n, got_s = R.ddpm_update(R.F32, i['x'], i['eps'], i['noise'], i['t'], tab, clamp=False)
    assert R.ratio(got_s, ref_s, s_s) > R.K_XS and R.ratio(got_n, ref_n, s_n) > R.K_DDPM_NOISE
    ref_n, ref_s = R.ddim_update(R.F64, i['x'], i['eps'], i['noise'], i['t'], tab, coef)
    s_n, s_s = R.ddim_scale(i['x'], i['eps'], i['noise'], i['t'], tab, coef)
    got_n, got_s = R.ddim_update(R.F32, i['x'], i['eps'], i['noise'], i['t'], tab, coef, clamp=False)
    assert R.ratio(got_s, ref_s, s_s) > R.K_XS and R.ratio(got_n, ref_n, s_n) > R.K_DDIM


# ------------------------------------------------------------------------------------------------------------------ plans (no device needed)
@pytest.mark.parametrize('name', list(R.COND_BY_NAME))
def test_cond_case_reaches_its_form(K, name):
    c = R.COND_BY_NAME[name]
    for p in R.cond_plans(K, c).values():
        assert p['rc'] == 0 and R.plan_tuple(p) == c['expect'], p
    if name.startswith('rounds'):
        n = c['total'] // 4 if c['expect'][0] == 'float4' else c['total']
        assert c['expect'][1] == 2048 and R.rounds(n, 2048) == (2, True) and n > 2048 * 256


@pytest.mark.parametrize('name', list(R.LOSS_BY_NAME))
def test_loss_case_reaches_its_form(K, name):
    c = R.LOSS_BY_NAME[name]
    for arm, p in R.loss_plans(K, c).items():
        assert p['rc'] == 0 and R.plan_tuple(p) == R.loss_expect(c, arm), (arm, p)
    if name.startswith('rounds'):
        assert R.rounds(c['per_sample'] // 4, c['fwd'][1]) == (2, True) and R.rounds(c['per_sample'] // 4, c['bwd'][1]) == (2, True)


@pytest.mark.parametrize('name', list(R.UPDATE_BY_NAME))
def test_update_case_reaches_its_form(K, name):
    c = R.UPDATE_BY_NAME[name]
    for _, operands, _ in R.UPDATE_ARMS.values():
        p = R.update_plan(K, c, operands)
        assert p['rc'] == 0 and R.plan_tuple(p) == R.update_expect(c, operands), p
    if name.startswith('rounds'):
        assert R.rounds(c['per_sample'] // 4, c['expect'][1]) == (2, True)


def test_plans_report_refusals(K):
    """rc is the code the launch would return; the other fields are 0 then"""
    from wdno_amd._lib import CondDesc
    ok = R.cond_desc_of(K, R.COND_BY_NAME['smoke-w8-C42-pad'])
    for edit in (dict(tree=2), dict(tree=1), dict(W=0), dict(B=0)):
        d = CondDesc.from_buffer_copy(bytes(ok))
        for k, v in edit.items():
            setattr(d, k, v)
        p = K.cond_plan(d)
        assert (p['rc'], p['form'], p['grid_x'], p['grid_y']) == (R.WDNO_EINVAL, None, 0, 0), (edit, p)
    assert K.weighted_mse_plan(3, 520, 5, 52, ws_bytes=7 * 8)['rc'] == 0
    assert K.weighted_mse_plan(3, 520, 5, 52, ws_bytes=7 * 8 - 1)['rc'] == R.WDNO_EWORKSPACE
    assert K.weighted_mse_plan(3, 520, 5, 52, ws_bytes=0, backward=True)['rc'] == 0         # the backward has no workspace
    assert K.weighted_mse_plan(0, 520, 5, 52)['rc'] == R.WDNO_EINVAL and K.weighted_mse_plan(3, 520, 0, 52)['rc'] == R.WDNO_EINVAL
    assert K.update_plan(0, 4)['rc'] == R.WDNO_EINVAL and K.update_plan(3, 0)['rc'] == R.WDNO_EINVAL
    assert K.update_plan(65535, 4)['form'] == 'float4' and K.update_plan(65536, 4)['form'] == 'scalar'
    assert K.weighted_mse_plan(2048, 256, 2, 64, backward=True)['form'] == 'float4' and K.weighted_mse_plan(2049, 256, 2, 64, backward=True)['form'] == 'scalar'
    assert K.cond_plan(ok, 8)['form'] == 'scalar' and K.cond_plan(ok, 16)['form'] == 'float4'      # only the low four bits count


def test_coverage(K):
    """the matrix reaches every kernel of the unit in every arm (R.check_coverage, shared with the GPU test)"""
    print(R.check_coverage(K))
