"""Inputs of the Burgers cascade fixture (tests/golden/ref_burgers_cascade.npz), regenerated identically by the fixture generator
(tests/golden/make_ref_burgers_cascade_golden.py) and by the tests from the integer hash of tests/helpers.py, so that the fixture stores only
what the reference computed. No product code here.

The run: evaluate() with upsample_x = upsample_t = 2, a batch of 2, conditioned on u0 and uT. The test file holds smooth fields u [2, 321, 480]
and f [2, 320, 480]. The sample a level's model returns is built like tests/burgers_eval_inputs.case_input: the packed transform of smooth
fields inside the level's coefficient block, divided by RESCALER, and dense junk everywhere else (padding, the low and condition channels),
which a correct reconstruction never reads."""
import numpy as np
import torch

from oracle import dwt_ref as R
from tests.burgers_eval_inputs import smooth
from tests.helpers import _hash_values

WAVE, MODE = 'bior2.4', 'periodization'
B, UPSAMPLE = 2, 2
WF = 0.03
RESCALER = [10, 3, 3, 1, 21, 5, 5, 1] * 2 + [10]             # eval_ddpm_burgers.py:391-405 with is_super_model and a condition channel
SHAPES = [[41, 60], [81, 120], [161, 240]]                   # coefficient block of level k
ORI = [[81, 120], [161, 240], [321, 480]]                    # field size of level k
CHANNELS = [9, 17, 17]
# the solver call the wrappers make in place of T = 8: T = 0.1 is 7 680 steps, the level's record count, the full grid
SOLVER = [dict(T=0.1, num_t=80 * 2 ** k, s=1920) for k in range(3)]
# rows of the condition channel that the fixture stores in full: first and last row of every stripe (P = 64 2^k, rep = P / 4)
cond_rows = lambda P: sorted({s * (P // 4) + o for s in range(4) for o in (0, P // 4 - 1)})
LOW_STEP = (3, 5)                                            # low is stored at rows ::3 and columns ::5 of its box: both copies of a coefficient


def super_test_file():
    """{'u': [2, 321, 480], 'f': [2, 320, 480]} fp32: the super-resolution test file."""
    return {'u': torch.from_numpy(smooth(B, 321, 480, 901, amp=0.4, knots=(4, 7))).float(),
            'f': torch.from_numpy(smooth(B, 320, 480, 902, amp=0.3, knots=(7, 5))).float()}


def rescaler(k):
    """RESCALER of level k as evaluate() passes it: [1, 9, 1, 1] (entries 8..16) at the base level, [1, 17, 1, 1] above."""
    r = np.asarray(RESCALER[8:] if k == 0 else RESCALER, dtype=np.float64)
    return torch.from_numpy(r.reshape(1, -1, 1, 1)).float()


def sample_output(k):
    """What the recorder model of level k returns from sample(): [2, C, 64 2^k, 64 2^k] fp32 in network units."""
    (h, w), (n_t, n_x), ch, P, seed = SHAPES[k], ORI[k], CHANNELS[k], 64 * 2 ** k, 910 + 10 * k
    u = smooth(B, n_t, n_x, seed)
    f = smooth(B, n_t, n_x, seed + 1, knots=(7, 5))
    f[:, n_t - 1] = 0.0
    yl, yh = R.dwt2(np.stack((u, f), axis=1), WAVE, MODE)
    assert yl.shape[-2:] == (h, w)
    r = rescaler(k).double().numpy().reshape(-1)
    x = 0.6 * _hash_values(B * ch * P * P, seed + 2).reshape(B, ch, P, P)
    x[:, :8, :h, :w] = R.burgers_coef_to_tensor(yl, yh).reshape(B, 8, h, w) / r[:8].reshape(1, 8, 1, 1)
    return torch.from_numpy(x).float()


def small_case(b, seed=77):
    """The smallest shapes at which the hand-off can go wrong: previous block (9, 13), fine block (17, 26), P_t = 20, P_x = 28 -- 18 copied
    rows against 17, rows of 112 bytes, P_t != P_x, stripes of 5 rows against tiles of 16. Returns x_prev [b, 8, 9, 13], the target
    [b, 33, 52] and RESCALER [17] (fp32), all dense."""
    x = torch.from_numpy(2.0 * _hash_values(b * 8 * 9 * 13, seed).reshape(b, 8, 9, 13)).float()
    t = torch.from_numpy(smooth(b, 33, 52, seed + 1, amp=0.5, knots=(5, 9))).float()
    return x, t, torch.linspace(1.0, 9.0, 17)
