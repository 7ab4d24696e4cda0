"""The metrics of the Burgers evaluation on the GPU: mse_deviation and the two metric(..., evaluate=True) calls of diffuse_2dconv
(eval_ddpm_burgers.py:220-230, test_util.py:23-30, 79-98) as one launch of csrc/burgers_score.hip (include/wdno_hip.h: wdno_burgers_score)
and one device-to-host copy of its 14 fp64 numbers per sample.

The reference runs, per batch, a clone of every operand, u_repeat (an expand and a copying reshape), two metric() calls with two sorts each
for the medians and a dozen reductions, and five .cpu() synchronisations. Here x_gt and u_target are read in place as strided views (the
solver's output, or the target cropped to the field's columns), u_repeat is never formed, and the medians are selected exactly in LDS.

sums()    -- the launch: out [B, 14] fp64 on the GPU (the columns are those of include/wdno_hip.h).
formulas()-- numpy fp64, pure host: the reference's metric formulas on such an array.
score()   -- sums(), one copy, formulas().

nmse and nmae are reproduced as the reference has them (test_util.py:87-88), with two things to know about them: their normaliser is a
mean over the WHOLE BATCH (sqrt(mean over batch and columns of t^2) + 1e-5, and the same with |t|), formed here from the per-sample sums of
t^2 and |t|, so a sample's nmse / nmae depend on which other samples share its batch; and nmae takes the square root of the mean absolute
error. The arrays are float64 where the reference has float32.
"""
import ctypes as C

import numpy as np
import torch

COLUMNS = ('ddpm', 'u_sq_strided', 'u_sq', 'u_abs', 'u_sq_median', 'u_abs_median', 'gt_sq_strided', 'gt_sq', 'gt_abs', 'gt_sq_median',
           'gt_abs_median', 'f_sq', 't_sq', 't_abs')
METRICS = ('mse', 'mse_median', 'mae', 'mae_median', 'nmse', 'nmae')
MAX_WIDTH = 3840            # n_x sub: the two fp64 rows the medians are selected from fit 64 KiB of LDS


def lower_median_rank(n):
    """torch.median of a row of n values returns the element of this rank of the sorted row (the lower of the two middle ones)."""
    return (n - 1) // 2


def _view_strides(t, what, shape):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != tuple(shape):
        raise ValueError(f'burgers score: {what} must be a float32 {tuple(shape)} tensor on the GPU, got '
                         f'{getattr(t, "dtype", type(t))} {tuple(getattr(t, "shape", ()))}')
    st = [0 if n == 1 else int(s) for n, s in zip(t.shape, t.stride())]
    if min(st) < 0:
        raise ValueError(f'burgers score: {what} has a negative stride')
    return st


def sums(u, f, x_gt, u_target):
    """out [B, 14] fp64 on u's device. u [B, n_t, n_x], f [B, n_t - 1, n_x] fp32 on the GPU; x_gt, u_target fp32 views [B, n_t, n_x sub]."""
    from wdno_amd import _lib
    from wdno_amd.ops import _p, _stream
    if not u.is_cuda or u.dtype != torch.float32 or u.dim() != 3:
        raise RuntimeError(f'burgers score: u must be a float32 [B, n_t, n_x] tensor on the GPU, got {u.dtype} {tuple(u.shape)} on {u.device}')
    B, n_t, n_x = (int(v) for v in u.shape)
    if f.dtype != torch.float32 or tuple(f.shape) != (B, n_t - 1, n_x) or f.device != u.device:
        raise ValueError(f'burgers score: f must be a float32 {(B, n_t - 1, n_x)} tensor on {u.device}, got {f.dtype} {tuple(f.shape)}')
    sub = int(x_gt.shape[-1]) // n_x
    if sub < 1 or n_x * sub > MAX_WIDTH:
        raise ValueError(f'burgers score: x_gt is {x_gt.shape[-1]} wide; between {n_x} and {MAX_WIDTH} columns are taken')
    u, f = u.detach().contiguous(), f.detach().contiguous()
    x_gt, u_target = x_gt.detach(), u_target.detach()
    gs = _view_strides(x_gt, 'x_gt', (B, n_t, n_x * sub))
    ts = _view_strides(u_target, 'u_target', (B, n_t, n_x * sub))
    if x_gt.device != u.device or u_target.device != u.device:
        raise ValueError('burgers score: all operands must live on one device')
    with torch.cuda.device(u.device):
        out = torch.empty(B, 14, dtype=torch.float64, device=u.device)
        desc = _lib.BurgersScoreDesc(B, n_t, n_x, sub, gs[0], gs[1], gs[2], ts[0], ts[1], ts[2], 16 * n_x * sub, 0)
        _lib.check(_lib.load().wdno_burgers_score(_p(u), _p(f), _p(x_gt), _p(u_target), _p(out), C.byref(desc), _stream()), 'wdno_burgers_score')
    return out


def _candidate(s, k, n_x, nw, report_all):
    mse = s[:, k] / n_x
    if not report_all:
        return mse
    ep = 1e-5
    b = s.shape[0]
    nmse = np.sqrt(s[:, k + 1] / nw) / (np.sqrt(s[:, 12].sum() / (b * nw)) + ep)
    nmae = np.sqrt(s[:, k + 2] / nw) / (np.sqrt(s[:, 13].sum() / (b * nw)) + ep)
    return np.stack((mse, s[:, k + 3], s[:, k + 2] / nw, s[:, k + 4], nmse, nmae))


def formulas(s, n_t, n_x, sub, wf, upsample_t=0, report_all=True, actual_is_diffused=False):
    """The reference's numbers from the sums s [B, 14] (numpy fp64): ddpm_mse [B], J_diffused and J_actual ((6, B) in the order of METRICS
    when report_all, else (B,) holding mse), energy [B], total_J [B]. actual_is_diffused: is_condition_f, where the reference scores
    u_repeat twice (eval_ddpm_burgers.py:227-228)."""
    s = np.asarray(s, dtype=np.float64)
    nw = n_x * sub
    ddpm_mse = s[:, 0] / ((n_t - 1) * n_x)
    j_diffused = _candidate(s, 1, n_x, nw, report_all)
    j_actual = j_diffused.copy() if actual_is_diffused else _candidate(s, 6, n_x, nw, report_all)
    energy = s[:, 11] / (2 ** upsample_t) ** 2
    mse_actual = j_actual[0] if report_all else j_actual
    return ddpm_mse, j_diffused, j_actual, energy, mse_actual + wf * energy


def score(u, f, x_gt, u_target, wf, upsample_t=0, report_all=True, actual_is_diffused=False):
    """(ddpm_mse, J_diffused, J_actual, energy, total_J) as numpy fp64 arrays: one launch, one device-to-host copy. See formulas() and the
    module docstring for nmse / nmae."""
    n_t, n_x = int(u.shape[1]), int(u.shape[2])
    s = sums(u, f, x_gt, u_target).cpu().numpy()
    return formulas(s, n_t, n_x, int(x_gt.shape[-1]) // n_x, wf, upsample_t, report_all, actual_is_diffused)
