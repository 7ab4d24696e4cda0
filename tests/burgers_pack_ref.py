"""Host evaluation of the packed state of the Burgers wavelet models (get_wavelet_super_preprocess, wdno_pack_burgers_state) by the oracle: plain
indexing for the coefficient channels, oracle.dwt_ref.idwt2 / dwt1d for the two rows of u behind the condition channel. dtype float64 is the exact
value of the chain on the given fp32 coefficients (the arbiter of the gates), float32 the reference's own arithmetic where no recorded output
exists. Test infrastructure only."""
import numpy as np

from oracle import dwt_ref as R


def packed_state(fine, coarse, rescaler, ori_shape, pad_t, pad_x, wave='bior2.4', u0=True, uT=True, idx=None, dtype=np.float64):
    """fine [N, 2, 4, nt, nx], coarse [N, 2, 4, nt_c, nx_c] or None, rescaler scalar or C values, ori_shape = (ori_t, ori_x) of the level
    -> [B, 8 + 8 has_low + has_cond, pad_t, pad_x] in `dtype`."""
    fine = np.asarray(fine, dtype=dtype)
    coarse = None if coarse is None else np.asarray(coarse, dtype=dtype)
    if idx is not None:
        fine = fine[list(idx)]
        coarse = None if coarse is None else coarse[list(idx)]
    b, nt, nx = fine.shape[0], fine.shape[-2], fine.shape[-1]
    c = 8 + (8 if coarse is not None else 0) + (1 if (u0 or uT) else 0)
    out = np.zeros((b, c, pad_t, pad_x), dtype=dtype)
    out[:, :8, :nt, :nx] = fine.reshape(b, 8, nt, nx)
    if coarse is not None:
        out[:, :8, nt] = out[:, :8, nt - 1]
        up = R.upsample_coef_2d(coarse.reshape(b, 8, *coarse.shape[-2:]))
        out[:, 8:16, :up.shape[-2], :up.shape[-1]] = up
    if u0 or uT:
        ori_t, ori_x = int(ori_shape[0]), int(ori_shape[1])
        u = R.idwt2(fine[:, :1, 0], fine[:, :1, 1:4], wave, 'periodization')[:, 0, :ori_t, :ori_x]
        lo, hi = R.dwt1d(u[:, [0, ori_t - 1]], wave, 'periodization')                  # [B, 2, nx] each
        rep = pad_t // 4
        if u0:
            out[:, -1, :rep, :nx] = lo[:, None, 0]
            out[:, -1, rep:2 * rep, :nx] = hi[:, None, 0]
        if uT:
            out[:, -1, 2 * rep:3 * rep, :nx] = lo[:, None, 1]
            out[:, -1, 3 * rep:4 * rep, :nx] = hi[:, None, 1]
    r = np.asarray(rescaler, dtype=np.float32).astype(dtype).reshape(-1)
    return out / (r if r.size == 1 else r.reshape(1, c, 1, 1))


def channel_error(got, exact):
    """max-abs over the channel, divided by the channel's max"""
    exact = np.asarray(exact, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - exact).max() / np.abs(exact).max())
