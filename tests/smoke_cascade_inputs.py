"""Inputs of the smoke cascade fixture (tests/golden/ref_smoke_cascade_*.npz), regenerated identically by the fixture generator
(tests/golden/make_ref_smoke_cascade_golden.py) and by the tests from the integer hash of tests/helpers.py, so that the fixture stores
outputs only; and the fp64 evaluations the GPU gates compare against. Test infrastructure, no product code."""
import numpy as np
import torch

from tests.helpers import _hash_values

W_ENERGY = 0.7
PAD_T, PAD_X = 24, 80                                     # the super level's tensor (inference_2d.py:176)
# name: batch, coefficient blocks and field sizes per level, seed. The base tensor is [B, 24, 42, 40, 40], the super one [B, 24, 82, 80, 80].
CASES = {
    'small': dict(batch=2, shape=[(10, 18, 18), (10, 34, 34)], ori=[(16, 32, 32), (16, 64, 64)], seed=301),
    'full': dict(batch=1, shape=[(18, 34, 34), (18, 66, 66)], ori=[(32, 64, 64), (32, 128, 128)], seed=402),
}
FILE_COND = lambda name: f'ref_smoke_cascade_{name}_cond.npz'
FILE_PRED = lambda name, level: f'ref_smoke_cascade_{name}_pred{level}.npz'
FILE_SCORE = 'ref_smoke_cascade_score.npz'
PRED_FRAMES = lambda to: [0, 1, to // 2, to - 1]          # frames of channels 0..4 of pred the fixture stores, rows ::PRED_ROWS
PRED_ROWS = 3
LOW_FRAMES = lambda t0: [0, t0 // 2, t0 - 1]              # low: these frames, channels ::LOW_CHANNELS, rows ::LOW_ROWS of the up-sampled block
LOW_CHANNELS, LOW_ROWS = 4, 4
INIT_FRAMES = (0, 1, 2, 3, 4, 5, 6, 7, 23)                # init: the block plus one zero row and column
CONTROL_FRAMES = lambda t1: [0, 1, t1 // 2, t1 - 1]       # control: these frames, rows CONTROL_ROWS(h1), the block with its rim plus one zero column
CONTROL_ROWS = lambda h1: sorted(set(range(0, h1 + 3, 4)) | {0, 1, h1 + 1, h1 + 2})
SCORE_B, SCORE_T, SCORE_N = 2, 4, 128                     # the scoring cases: pred 64 x 64 (level 0) and 128 x 128 (level 1), data 128 x 128


def rescaler():
    """RESCALER [1, 1, 82, 1, 1] of the super model (fp32)."""
    return torch.linspace(1.0, 9.0, 82).reshape(1, 1, 82, 1, 1)


def fine_state(name):
    """The batch a dataloader hands to run_model in simulation mode: [B, to, 6, 2 ho, 2 wo] fp32, a hash plus a ramp."""
    c = CASES[name]
    b, (to, ho, wo) = c['batch'], c['ori'][1]
    v = _hash_values(b * to * 6 * ho * wo, c['seed'] + 7).reshape(b, to, 6, ho, wo) + np.linspace(-0.5, 0.5, wo).reshape(1, 1, 1, 1, wo)
    return torch.from_numpy(v).float()


def sample_output(name, level):
    """What the stub model of `level` returns from sample(): a DENSE x [B, 24, 42 or 82, 40 or 80, .] in network units, so that a block read
    at a wrong offset, or smoke-out rows split at a wrong row, give other values."""
    c = CASES[name]
    tshape = (c['batch'], PAD_T, 42 + 40 * level, 40 * 2 ** level, 40 * 2 ** level)
    return torch.from_numpy(0.6 * _hash_values(int(np.prod(tshape)), c['seed'] + level).reshape(tshape)).float()


def score_pred(level):
    n = 64 * 2 ** level
    return torch.from_numpy(_hash_values(SCORE_B * SCORE_T * 6 * n * n, 511 + level).reshape(SCORE_B, SCORE_T, 6, n, n)).float()


def score_data():
    return torch.from_numpy(_hash_values(SCORE_B * SCORE_T * 6 * SCORE_N * SCORE_N, 523).reshape(SCORE_B, SCORE_T, 6, SCORE_N, SCORE_N)).float()


def level_rescaler(level):
    """The values a level's sample is multiplied by (inference_2d.py:215, 224): entries :40 and -1 of the 82 (what lies between is not read)."""
    r = rescaler().reshape(-1)
    return r if level else torch.cat((r[:41], r[-1:]))


def exact_pred(x, resc, shape, ori, half, off):
    """pred [B, to, 6, ho, wo] of one cascade level (inference_2d.py:213-231) in fp64 by oracle/dwt_ref.py from the fp32 sample and the level's
    rescaler: the coefficient block at rows and columns off .., the smoke-out means over the whole rows [:half] / [half:]."""
    from oracle import dwt_ref as R
    xs = x.double().numpy() * resc.double().numpy().reshape(1, 1, -1, 1, 1)
    (tc, hc, wc), (to, ho, wo) = shape, ori
    out = np.zeros((xs.shape[0], to, 6, ho, wo))
    for f in range(5):
        blk = xs[:, :tc, 8 * f:8 * f + 8, off:off + hc, off:off + wc].transpose(0, 2, 1, 3, 4)
        rec = R.idwt3(blk[:, 0], {k: blk[:, i] for i, k in enumerate(R.BANDS3) if i}, 'bior1.3')
        out[:, :, f] = rec[:, :to, :ho, :wo]
    lo, hi = xs[:, :tc, -1, :half].mean((-2, -1)), xs[:, :tc, -1, half:].mean((-2, -1))
    out[:, :, 5] = R.idwt1d(lo[:, None], hi[:, None], 'bior1.3', 'zero')[:, 0, :to, None, None]
    return out


def bilinear2x(p):
    """F.interpolate(p, scale 2, mode='bilinear', align_corners=False) on the last two axes in numpy (the dtype of p): the source coordinate of
    output y is y / 2 - 0.25 clamped at 0, so even rows are 0.25 p[k - 1] + 0.75 p[k], odd rows 0.75 p[k] + 0.25 p[k + 1], indices clamped."""
    def axis(a, ax):
        a = np.moveaxis(a, ax, -1)
        n = a.shape[-1]
        k = np.arange(n)
        out = np.empty(a.shape[:-1] + (2 * n,), dtype=a.dtype)
        out[..., 0::2] = 0.25 * a[..., np.maximum(k - 1, 0)] + 0.75 * a
        out[..., 1::2] = 0.75 * a + 0.25 * a[..., np.minimum(k + 1, n - 1)]
        return np.moveaxis(out, -1, ax)
    return axis(axis(p, -1), -2)


def super_views(pred, data):
    """The four (pred, data) pairs of multi_evaluate's super-resolution branch in simulation mode (inference_2d.py:405-421), numpy."""
    n, N = pred.shape[-1], data.shape[-1]
    f = N // n
    up = (lambda a: a) if f == 1 else bilinear2x
    near = (lambda a: a) if f == 1 else (lambda a: a.repeat(2, axis=-2).repeat(2, axis=-1))
    sp = n // (N // 2)
    return [(pred[..., ::sp, ::sp], data[..., ::2, ::2]), (pred, data[..., ::f, ::f]), (up(pred), data), (near(pred), data)]


def metrics_super_fp64(pred, data, w_energy):
    """{key: [4, B]} of the four comparisons in plain numpy fp64 (tests/smoke_inference_inputs.metrics_fp64 on each pair)."""
    from tests.smoke_inference_inputs import metrics_fp64
    rows = [metrics_fp64(p, d, w_energy) for p, d in super_views(np.array(pred, dtype=np.float64), np.array(data, dtype=np.float64))]
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}
