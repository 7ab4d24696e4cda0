"""The wavelet kernels (csrc/dwt.hip, csrc/dwt_analysis.hip, csrc/dwt_synthesis.hip) held ELEMENT BY ELEMENT to the fp64 reference of
tests/dwt_kernels_ref.py, |got - ref| <= K 2^-24 S_e with K = nd (L + 1) + 1 and S_e the same transform of |input| with |taps| (exactly 0 where
S_e = 0), on a case matrix chosen by launch regime: every kernel instantiation the choosers can launch, every width fall-back, both block-count
classes of xcd_tile, random taps without symmetry (a reversed, shifted or swapped tap moves every output), filters up to 16 taps, the smallest
legal periodization sizes, padded coefficient tensors and the packed analysis. K and the reference are anchored on the CPU
(tests/test_host_dwt_kernels_ref.py), not on the kernels. Per case: ops.dwt_plan says the case reaches the regime it exists for and asks for no
more than 64 KB of LDS; the four entry points are gated through ops.dwt_call (raw taps, strides); a second run gives equal bits; where the plan
says fused the per-axis passes (debug mode 11) give equal bits, and for the 3-D synthesis so does the other fused kernel (debug mode 45)."""
import numpy as np
import pytest
import torch

from tests import dwt_kernels_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def ops():
    from wdno_amd import ops as o
    o._lib_()
    return o


def _call(ops, c, entry, src_np, taps):
    """one launch of `entry`: (the raw destination buffer, the result gathered to its dense shape). The coefficient tensor is a flat buffer
    with the case's strides: SENTINEL in its padding as a destination, NaN in its padding as a source (a kernel that folds padding into a sum
    shows). A signal destination is pre-filled with NaN: every sample has to be written."""
    nd, mode, L, n_img, ind, outd, cs = R.desc_args(c, entry)
    sig, cdims = R.geometry(c, entry)
    off = torch.from_numpy(R.coef_offsets(n_img, nd, cdims, cs).reshape(-1)).to(DEV)
    if entry in R.ANALYSIS_SHAPED:
        src = torch.from_numpy(src_np).to(DEV).contiguous()
        dst = torch.full((n_img * cs[0],), R.SENTINEL, device=DEV)
        ops.dwt_call(entry, src, dst, nd, mode, taps, n_img, ind, outd, cs)
        pad = torch.ones_like(dst, dtype=torch.bool)
        pad[off] = False
        assert bool((dst[pad] == R.SENTINEL).all()), f'{entry}: padding of the coefficient tensor written'
        return dst, dst[off].reshape(n_img, 2 ** nd, *cdims)
    src = torch.full((n_img * cs[0],), float('nan'), device=DEV)
    src[off] = torch.from_numpy(src_np).to(DEV).reshape(-1)
    dst = torch.full((n_img, *sig), float('nan'), device=DEV)
    ops.dwt_call(entry, src, dst, nd, mode, taps, n_img, ind, outd, cs)
    return dst, dst


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('name', list(R.BY_NAME))
def test_dwt_gate(ops, name):
    c = R.BY_NAME[name]
    lib = ops._lib
    taps_np = R.bank_of(c)
    taps = R.flat_taps(taps_np)
    K = R.gate_k(c['nd'], c['L'])
    plans = R.plans_of(ops, c)
    for e, p in plans.items():                                                # 1. the regime: kernel, tile geometry, blocks, LDS
        R.check_plan(c, e, p)
    worst = {}
    for entry in R.ENTRIES:
        sig, _ = R.geometry(c, entry)
        for variant in c['variants']:
            src = R.make_input(R.src_shape(c, entry), c['nd'], c['L'], variant, R.case_seed(c, entry, variant))
            with lib.debug_mode(c['debug']):
                raw, got = _call(ops, c, entry, src, taps)                        # 2. run
                raw2, _ = _call(ops, c, entry, src, taps)                         # 4. again
            ref, scale = R.reference(entry, src, taps_np, c['mode'], c['nd'], sig)
            r = R.ratio(got.cpu().numpy(), ref, scale) / K                        # 3. the gate
            worst[entry] = max(worst.get(entry, 0.0), r)
            assert r <= 1.0, (entry, variant, r)
            assert _same_bits(raw, raw2), (entry, variant, 'second run')
            if plans[entry]['family'] != 'per_axis':                              # 5. the per-axis passes, the other 3-D synthesis kernel
                with lib.debug_mode(R.DBG_PER_AXIS_DWT):
                    assert ops.dwt_plan(entry, *R.desc_args(c, entry))['family'] == 'per_axis'
                    raw11, _ = _call(ops, c, entry, src, taps)
                assert _same_bits(raw, raw11), (entry, variant, 'per-axis passes')
                if c['nd'] == 3 and entry not in R.ANALYSIS_SHAPED:
                    other = R.DBG_DWT3_SYNTH_LDS if not c['debug'] else 0
                    with lib.debug_mode(other):
                        fam = ops.dwt_plan(entry, *R.desc_args(c, entry))['family']
                        raw45, _ = _call(ops, c, entry, src, taps)
                    assert fam in ('synthesis_fused', 'synthesis3_stream', 'per_axis') and _same_bits(raw, raw45), (entry, variant, fam)
    print(f'{name} [{c["regime"]}] K {K}: ratio / K  ' + '  '.join(f'{e} {plans[e]["family"]}/{plans[e]["variant"]} {worst[e]:.3f}' for e in R.ENTRIES))


@pytest.mark.parametrize('name', list(R.PACKED_BY_NAME))
def test_packed_analysis_gate(ops, name):
    """wdno_dwt_fwd_packed: img_inner > 1, row_w > Wo and % 4 == 0, a distinct rescaler per (inner, band), rows longer than row_w: coefficient /
    rescaler within K + 1, exactly 0 from Wo to row_w, the sentinel everywhere else; equal bits on a second run and against wdno_dwt_fwd's
    coefficients divided by torch"""
    import ctypes as C
    c = R.PACKED_BY_NAME[name]
    lib = ops._lib_()
    taps_np, resc = R.bank_of(c), R.packed_rescaler(c)
    taps = R.flat_taps(taps_np)
    cdims, row_w, cs_outer, cs, total = R.packed_layout(c)
    p = R.packed_plan(ops, c)
    assert p['rc'] == 0 and p['family'] == 'analysis_packed' and p['lds_bytes'] <= 65536, p
    K = R.gate_k(3, c['L'], packed=True)
    off = torch.from_numpy(R.packed_offsets(c['n_img'], c['img_inner'], cdims, row_w, cs_outer, cs).reshape(-1)).to(DEV)
    d = ops._dwt_desc(3, 1, c['L'], c['n_img'], list(c['sig']), cdims, cs)
    fl = (C.c_float * len(taps))(*taps)
    rs = torch.from_numpy(resc).to(DEV)
    worst = 0.0
    for variant in ('gauss', 'wide', 'edge'):
        x_np = R.make_input((c['n_img'], *c['sig']), 3, c['L'], variant, 11)
        x = torch.from_numpy(x_np).to(DEV)
        states = []
        for _ in range(2):
            state = torch.full((total,), R.SENTINEL, device=DEV)
            ops._lib.check(lib.wdno_dwt_fwd_packed(ops._p(x), ops._p(state), C.byref(d), fl, c['img_inner'], cs_outer, row_w, ops._p(rs), ops._stream()),
                           'dwt_fwd_packed')
            states.append(state)
        state = states[0]
        assert _same_bits(state, states[1])
        pad = torch.ones_like(state, dtype=torch.bool)
        pad[off] = False
        assert bool(pad.any()) and bool((state[pad] == R.SENTINEL).all()), 'written outside the rows [k0 < To][k1 < Ho][k2 < row_w]'
        got = state[off].reshape(c['n_img'], 8, cdims[0], cdims[1], row_w)
        ref, scale = R.packed_reference(x_np, taps_np, list(c['sig']), c['img_inner'], row_w, resc)
        assert bool((got[..., cdims[2]:] == 0).all())
        r = R.ratio(got.cpu().numpy(), ref, scale) / K
        worst = max(worst, r)
        assert r <= 1.0, (variant, r)
        # the same bits as the unpacked transform divided by torch (IEEE division)
        dense = torch.empty((c['n_img'], 8, *cdims), device=DEV)
        ops.dwt_call('fwd', x, dense, 3, 1, taps, c['n_img'], list(c['sig']), cdims, R.coef_strides(3, cdims))
        div = dense / rs.reshape(c['img_inner'], 8)[torch.arange(c['n_img'], device=DEV) % c['img_inner']][:, :, None, None, None]
        assert _same_bits(got[..., :cdims[2]].contiguous(), div)
    print(f'{name} K {K}: ratio / K  fwd_packed {p["family"]} blocks {p["blocks"]} {worst:.3f}')


def test_coverage(ops):
    """the plans of the matrix reach every instantiation the choosers can launch and both block-count classes of every fused family; a retune
    of the heuristics has to revisit the matrix instead of silently emptying a regime"""
    print(R.check_coverage(ops))
