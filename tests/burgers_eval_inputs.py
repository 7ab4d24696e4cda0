"""Inputs of the Burgers evaluation fixtures (tests/golden/ref_burgers_eval.npz), regenerated identically by the fixture generator and by
the tests from an integer hash (tests/helpers._hash_values: no random generator, no libm), so only outputs are stored. No product code
here.

A case's x is what a sampler would return: the packed single-level forward transform (oracle/dwt_ref.dwt2, fp64) of smooth fields u and f
of amplitude 0.3, divided by RESCALER and rounded to fp32, inside the coefficient block; dense junk of amplitude 0.3 everywhere outside it
(rows and columns beyond the block, channels beyond the eighth), which a correct reconstruction never reads. Smooth means bilinear
interpolation of a coarse grid of hash values: arithmetic only."""
import numpy as np
import torch

from oracle import dwt_ref as R
from tests.helpers import _hash_values

RESCALER = [10, 3, 3, 1, 21, 5, 5, 1, 10]                    # eval_ddpm_burgers.py:391, 405 (bior2.4 / periodization, conditioned on u0 / uT)
WAVE, MODE = 'bior2.4', 'periodization'
WF = 0.03                                                    # the metric's energy weight in every case

# name: tensor shape, coefficient shape (padded_shape), field shape (ori_shape), RESCALER, and the solver call the test wrapper makes in
# place of T = 8: T = 0.1 is 7 680 steps; num_t records and s = 16 n_x grid points keep the reference's [:, :, ::16] the field's columns
CASES = {
    'full': dict(xshape=(2, 9, 64, 64), shape=(41, 60), ori=(81, 120), resc=RESCALER, solver=dict(T=0.1, num_t=80, s=1920)),
    'small': dict(xshape=(3, 8, 16, 24), shape=(9, 12), ori=(17, 24), resc=RESCALER[:8], solver=dict(T=0.1, num_t=16, s=384)),
}
SUB2 = dict(B=3, n_t=17, n_x=24, sub=2)                      # metric only, no solver: x_gt and u_target twice as wide as u


def seed_of(name):
    return sum(name.encode())


def smooth(b, rows, cols, seed, amp=0.3, knots=(5, 6)):
    """[b, rows, cols] fp64 in [-amp, amp): bilinear interpolation of a knots[0] x knots[1] grid of hash values."""
    kr, kc = knots
    g = 2.0 * amp * _hash_values(b * kr * kc, seed).reshape(b, kr, kc)
    pr = np.arange(rows, dtype=np.float64) * (kr - 1) / max(rows - 1, 1)
    pc = np.arange(cols, dtype=np.float64) * (kc - 1) / max(cols - 1, 1)
    r0, c0 = np.minimum(pr.astype(np.int64), kr - 2), np.minimum(pc.astype(np.int64), kc - 2)
    wr, wc = (pr - r0)[None, :, None], (pc - c0)[None, None, :]
    a = g[:, r0][:, :, c0] * (1 - wc) + g[:, r0][:, :, c0 + 1] * wc
    c = g[:, r0 + 1][:, :, c0] * (1 - wc) + g[:, r0 + 1][:, :, c0 + 1] * wc
    return a * (1 - wr) + c * wr


def case_input(name):
    """x [B, C, H, W] fp32 (network units), RESCALER [1, C, 1, 1] fp32, u_target_ori [B, n_t, n_x] fp32 (field units)."""
    c = CASES[name]
    b, ch, hh, ww = c['xshape']
    (h, w), (n_t, n_x), seed = c['shape'], c['ori'], seed_of(name)
    u = smooth(b, n_t, n_x, seed)
    f = smooth(b, n_t, n_x, seed + 1, knots=(7, 5))
    f[:, n_t - 1] = 0.0                                      # f has n_t - 1 rows; the transform sees a zero row (wave_trans.py:99-123)
    yl, yh = R.dwt2(np.stack((u, f), axis=1), WAVE, MODE)
    assert yl.shape[-2:] == (h, w)
    packed = R.burgers_coef_to_tensor(yl, yh).reshape(b, 8, h, w)
    r = np.asarray(c['resc'], dtype=np.float64)
    x = 0.6 * _hash_values(b * ch * hh * ww, seed + 2).reshape(b, ch, hh, ww)
    x[:, :8, :h, :w] = packed / r[:8].reshape(1, 8, 1, 1)
    u_target = smooth(b, n_t, n_x, seed + 3, amp=0.4, knots=(4, 7))
    return torch.from_numpy(x).float(), torch.from_numpy(r.reshape(1, ch, 1, 1)).float(), torch.from_numpy(u_target).float()


def sub2_input():
    """u [B, n_t, n_x], f [B, n_t - 1, n_x], x_gt and u_target [B, n_t, n_x sub], fp32."""
    b, n_t, n_x, sub = (SUB2[k] for k in ('B', 'n_t', 'n_x', 'sub'))
    seed = seed_of('sub2')
    mk = lambda *a, **k: torch.from_numpy(smooth(*a, **k)).float()
    return (mk(b, n_t, n_x, seed), mk(b, n_t - 1, n_x, seed + 1, knots=(7, 5)), mk(b, n_t, n_x * sub, seed + 2, knots=(6, 6)),
            mk(b, n_t, n_x * sub, seed + 3, amp=0.4, knots=(4, 7)))


def edge_input():
    """The hand-made reconstruction edge case: x [1, 8, 12, 20] dense, block (7, 9), field (13, 17), RESCALER linspace(1, 9, 8)."""
    x = 0.6 * _hash_values(8 * 12 * 20, 4711).reshape(1, 8, 12, 20)
    return torch.from_numpy(x).float(), torch.from_numpy(np.linspace(1.0, 9.0, 8)).float(), (7, 9), (13, 17)
