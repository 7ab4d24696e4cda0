"""Inputs of the smoke inference fixture (tests/golden/ref_smoke_inference*.npz), regenerated identically by the fixture generator and by
the tests from the integer hash of tests/helpers.py, so that the fixture stores outputs only. Test infrastructure, no product code."""
import numpy as np
import torch

from tests.helpers import _hash_values, guidance_input

W_ENERGY = 0.7
# name: (state tensor of the sampler, coefficient block, field size, is_condition_control, seed)
CASES = {
    'small_control': ((2, 12, 42, 40, 40), (10, 18, 18), (16, 32, 32), False, 101),
    'small_sim': ((2, 12, 42, 40, 40), (10, 18, 18), (16, 32, 32), True, 101),
    'full_sim': ((1, 24, 42, 40, 40), (18, 34, 34), (32, 64, 64), True, 202),
}
FILE_OF = {'small_control': 'ref_smoke_inference.npz', 'small_sim': 'ref_smoke_inference.npz', 'full_sim': 'ref_smoke_inference_1.npz'}
PRED_FRAMES = lambda to: [0, 1, to // 2, to - 1]          # frames of channels 0..4 of pred the fixture stores, rows ::PRED_ROWS
PRED_ROWS = 3
CONTROL_ROWS = 4                                          # rows ::CONTROL_ROWS of the control condition are stored
INIT_FRAMES = (0, 5, 6, 11, 12, 17, 18, 23)               # first and last frame of each sub-band's run of pad_t / 4 = 6 frames


def sample_output(name):
    """What the stub model's sample() returns: x [B, F, 42, H, W] in network units, and RESCALER [1, 1, 42, 1, 1] (fp32)."""
    tshape, shape, ori, _, seed = CASES[name]
    x, resc, _ = guidance_input(tshape, shape, ori, seed)
    return x, resc


def base_state(name):
    """The base-resolution state [B, to, 6, ho, wo] (fp32, smooth enough to look like fields: a hash plus a ramp)."""
    tshape, _, ori, _, seed = CASES[name]
    b, (to, ho, wo) = tshape[0], ori
    v = _hash_values(b * to * 6 * ho * wo, seed + 7).reshape(b, to, 6, ho, wo)
    v = v + np.linspace(-0.5, 0.5, wo).reshape(1, 1, 1, 1, wo)
    return torch.from_numpy(v).float()


def batch_state(name):
    """The `state` a dataloader hands to run_model, whose base resolution is base_state(name): control mode [B, 8 to, 6, ho, wo] (one frame
    in 8 is the base state, the others are zero), simulation mode [B, to, 6, 2 ho, 2 wo] (one cell in 4)."""
    s = base_state(name)
    b, to, _, ho, wo = s.shape
    if CASES[name][3]:
        full = torch.zeros(b, to, 6, 2 * ho, 2 * wo)
        full[:, :, :, ::2, ::2] = s
    else:
        full = torch.zeros(b, 8 * to, 6, ho, wo)
        full[:, ::8] = s
    return full


def score_pred(name):
    """The pred [B, to, 6, ho, wo] fp32 that is scored (a hash: the tests cannot reproduce the bits of the reference's own fp32 pred)."""
    tshape, _, ori, _, seed = CASES[name]
    b, (to, ho, wo) = tshape[0], ori
    return torch.from_numpy(_hash_values(b * to * 6 * ho * wo, seed + 11).reshape(b, to, 6, ho, wo)).float()


def score_data_sim(name):
    """Simulation mode: the test batch [B, to, 6, 128, 128] fp32 the prediction is compared with."""
    tshape, _, ori, _, seed = CASES[name]
    b, to = tshape[0], ori[0]
    return torch.from_numpy(_hash_values(b * to * 6 * 128 * 128, seed + 13).reshape(b, to, 6, 128, 128)).float()


def score_data_control(name):
    """Control mode: what the metrics read of a solver_out -- [B, to, 6, ho, wo], fp32-representable values in fp64; channel 5 (the smoke
    share) is one value per frame, as the solver writes it. solver_out[b, f, c, y, x] = this[b, f // (256 // to), c, y // 2, x // 2]."""
    tshape, _, ori, _, seed = CASES[name]
    b, (to, ho, wo) = tshape[0], ori
    v = _hash_values(b * to * 6 * ho * wo, seed + 17).reshape(b, to, 6, ho, wo).astype(np.float32).astype(np.float64)
    v[:, :, 5] = _hash_values(b * to, seed + 19).reshape(b, to, 1, 1) + 0.5          # kept in fp64: the solver's ratio is fp64
    return v


def metrics_fp64(pred, data, w_energy):
    """multi_evaluate's formulas (inference_2d.py:426-439) in plain numpy fp64 for pred, data [B, T, 6, h, w]: per-sample arrays."""
    p, d = np.array(pred, dtype=np.float64), np.array(data, dtype=np.float64)
    p[:, 0, 0] = 0.0
    d[:, 0, 0] = 0.0
    e = p - d
    ax = (1, 2, 3, 4)
    out = dict(mse=(np.concatenate((e[:, :, :3], e[:, :, 5:]), axis=2) ** 2).mean(ax), mse_wo_smoke=(e[:, :, :3] ** 2).mean(ax),
               n_l2=np.sqrt((e[:, :, :3] ** 2).sum(ax)) / np.sqrt((d[:, :, :3] ** 2).sum(ax)), J_target=-d[:, -1, -1, 0, 0],
               J_energy=(d[:, :, 3:5] ** 2).mean(ax))
    out['J_total'] = out['J_target'] + w_energy * out['J_energy']
    return out


def exact_pred(x, resc, shape, ori, half):
    """pred [B, to, 6, ho, wo] of run_base_model's wavelet branch in fp64 by oracle/dwt_ref.py, from the fp32 sample and RESCALER."""
    from oracle import dwt_ref as R
    xs = x.double().numpy() * resc.double().numpy().reshape(1, 1, -1, 1, 1)
    (tc, hc, wc), (to, ho, wo) = shape, ori
    out = np.zeros((xs.shape[0], to, 6, ho, wo))
    for f in range(5):
        blk = xs[:, :tc, 8 * f:8 * f + 8, :hc, :wc].transpose(0, 2, 1, 3, 4)
        rec = R.idwt3(blk[:, 0], {k: blk[:, i] for i, k in enumerate(R.BANDS3) if i}, 'bior1.3')
        out[:, :, f] = rec[:, :to, :ho, :wo]
    lo, hi = xs[:, :tc, -1, :half].mean((-2, -1)), xs[:, :tc, -1, half:].mean((-2, -1))
    out[:, :, 5] = R.idwt1d(lo[:, None], hi[:, None], 'bior1.3', 'zero')[:, 0, :to, None, None]
    return out
