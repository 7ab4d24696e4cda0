"""numpy fp64 evaluation of the Burgers evaluation's reconstruction and scoring on fp32 inputs: the exact value the GPU gates of
tests/test_gpu_burgers_eval.py measure against. Pinned to the fp64 run of the reference's own code stored in
tests/golden/ref_burgers_eval.npz by tests/test_host_burgers_eval.py (1e-12). Test infrastructure only; no product code here."""
import numpy as np

from oracle import dwt_ref as R

COLUMNS = ('ddpm', 'u_sq_strided', 'u_sq', 'u_abs', 'u_sq_median', 'u_abs_median', 'gt_sq_strided', 'gt_sq', 'gt_abs', 'gt_sq_median',
           'gt_abs_median', 'f_sq', 't_sq', 't_abs')


def _f64(t):
    return np.asarray(t.detach().cpu().numpy() if hasattr(t, 'detach') else t, dtype=np.float64)


def reconstruct(x, rescaler, shape, ori_shape, wave='bior2.4', mode='periodization'):
    """u [B, n_t, n_x], f [B, n_t - 1, n_x] in fp64 from the fp32 x and RESCALER (eval_ddpm_burgers.py:185-195)."""
    x, r = _f64(x), _f64(rescaler).reshape(-1)
    r = np.broadcast_to(r, (8,)) if r.size == 1 else r[:8]
    yl, yh = R.burgers_tensor_to_coef(x[:, :8] * r.reshape(1, 8, 1, 1), shape)
    u_f = R.idwt2(yl, yh, wave, mode)[:, :, :ori_shape[-2], :ori_shape[-1]]
    return u_f[:, 0], u_f[:, 1, :ori_shape[-2] - 1]


def lower_median(v):
    """torch.median along the last axis: the element of rank (n - 1) // 2 of the sorted row."""
    return np.sort(v, axis=-1)[..., (v.shape[-1] - 1) // 2]


def sums(u, f, x_gt, u_target):
    """The 14 per-sample numbers of include/wdno_hip.h: wdno_burgers_score, [B, 14] fp64."""
    u, f, x_gt, ut = _f64(u), _f64(f), _f64(x_gt), _f64(u_target)
    sub = x_gt.shape[-1] // u.shape[-1]
    t = ut[:, -1]
    out = np.zeros((u.shape[0], 14))
    out[:, 0] = np.square(u[:, 1:] - x_gt[:, 1:, ::sub]).sum((-1, -2))
    for k, c in ((1, np.repeat(u[:, -1], sub, axis=-1)), (6, x_gt[:, -1])):
        d = c - t
        out[:, k], out[:, k + 1], out[:, k + 2] = np.square(d[:, ::sub]).sum(-1), np.square(d).sum(-1), np.abs(d).sum(-1)
        out[:, k + 3], out[:, k + 4] = lower_median(np.square(d)), lower_median(np.abs(d))
    out[:, 11], out[:, 12], out[:, 13] = np.square(f).sum((-1, -2)), np.square(t).sum(-1), np.abs(t).sum(-1)
    return out


def metric(u_target, f, wf, u, upsample_t=0):
    """test_util.metric(..., report_all=True, evaluate=True) in fp64: ((6, B), energy [B], total_J [B])."""
    ut, f, uc = _f64(u_target), _f64(f), _f64(u)
    sub = uc.shape[-1] // f.shape[-1]
    d, t, ep = uc[:, -1] - ut[:, -1], ut[:, -1], 1e-5
    mse = np.square(d[:, ::sub]).mean(-1)
    J = np.stack((mse, lower_median(np.square(d)), np.abs(d).mean(-1), lower_median(np.abs(d)),
                  np.sqrt(np.square(d).mean(-1)) / (np.sqrt(np.square(t).mean()) + ep), np.sqrt(np.abs(d).mean(-1)) / (np.sqrt(np.abs(t).mean()) + ep)))
    energy = np.square(f).sum((-1, -2)) / (2 ** upsample_t) ** 2
    return J, energy, mse + wf * energy


def evaluate(u, f, x_gt, u_target, wf, actual_is_diffused=False):
    """What diffuse_2dconv reports for one batch, fp64: ddpm_mse [B], J_diffused (6, B), J_actual (6, B), energy [B], total_J [B]."""
    u, x_gt = _f64(u), _f64(x_gt)
    sub = x_gt.shape[-1] // u.shape[-1]
    ddpm = np.square(u[:, 1:] - x_gt[:, 1:, ::sub]).mean((-1, -2))
    u_repeat = np.repeat(u, sub, axis=-1)
    J_diffused, _, _ = metric(u_target, f, wf, u_repeat)
    J_actual, energy, total_J = metric(u_target, f, wf, u_repeat if actual_is_diffused else x_gt)
    return ddpm, J_diffused, J_actual, energy, total_J
