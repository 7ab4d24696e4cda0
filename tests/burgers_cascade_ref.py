"""numpy fp64 evaluation of the hand-off between two levels of the Burgers cascade (eval_ddpm_burgers.py:306-338, test_util.py:185-196) on
fp32 inputs: the exact value the GPU gates of tests/test_gpu_burgers_cascade.py measure against. Pinned to the fp64 run of the reference's
own get_target stored in tests/golden/ref_burgers_cascade.npz by tests/test_host_burgers_cascade.py (1e-12). Test infrastructure only."""
import numpy as np

from oracle import dwt_ref as R


def _f64(t):
    return np.asarray(t.detach().cpu().numpy() if hasattr(t, 'detach') else t, dtype=np.float64)


def low32(x_prev, rescaler):
    """low's box [B, 8, 2 h0, 2 w0] in fp32: nearest x2 of x_prev, then ONE fp32 division by RESCALER[8:16] -- the bits of the reference."""
    x = np.asarray(x_prev.detach().cpu().numpy() if hasattr(x_prev, 'detach') else x_prev, dtype=np.float32)
    r = np.asarray(_f64(rescaler).reshape(-1)[8:16], dtype=np.float32).reshape(1, 8, 1, 1)
    return np.repeat(np.repeat(x, 2, axis=2), 2, axis=3) / r


def condition(u_target, rescaler, w1, pad_t, pad_x, cond_u0=True, cond_uT=True, wave='bior2.4', mode='periodization'):
    """Channel 16 [B, pad_t, pad_x] in fp64: four stripes of pad_t / 4 rows with the low / high band of the 1-D analysis of rows 0 and -1 of
    u_target[:, :, :2 w1], divided by RESCALER[16]; zero beyond the band and for a stripe whose flag is off."""
    ut, r = _f64(u_target), _f64(rescaler).reshape(-1)
    lo, hi = R.dwt1d(ut[:, [0, -1], :2 * w1], wave, mode)
    nx, rep = lo.shape[-1], pad_t // 4
    out = np.zeros((ut.shape[0], pad_t, pad_x))
    for s, band, on in ((0, lo[:, 0], cond_u0), (1, hi[:, 0], cond_u0), (2, lo[:, 1], cond_uT), (3, hi[:, 1], cond_uT)):
        if on:
            out[:, s * rep:(s + 1) * rep, :nx] = band[:, None] / r[16]
    return out


def conditions(x_prev, u_target, rescaler, shape1, pad_t, pad_x, cond_u0=True, cond_uT=True, wave='bior2.4', mode='periodization'):
    """The whole condition source [B, 17, pad_t, pad_x] in fp64 (low from the fp32 division: it is exact index work plus one rounding)."""
    low = low32(x_prev, rescaler)
    src = np.zeros((low.shape[0], 17, pad_t, pad_x))
    src[:, 8:16, :low.shape[2], :low.shape[3]] = low
    src[:, 16] = condition(u_target, rescaler, int(shape1[-1]), pad_t, pad_x, cond_u0, cond_uT, wave, mode)
    return src
