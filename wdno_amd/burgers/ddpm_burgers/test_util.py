"""MI355X drop-in for burgers/ddpm_burgers/test_util.py: the metrics, targets and model loaders of the Burgers evaluation.

Same names and signatures as the reference: SOLVER_N_UPSAMPLE, mse_deviation, metric, ddpm_guidance_loss, get_target,
load_burgers_dataset, load_burgers_dataset_wavelet, load_2dconv_base_model, load_2dconv_super_model, get_2d_ddpm (the reference imports
it from train_ddpm_burgers.py:128-182; it is defined here, on this tree's Unet2D / GaussianDiffusion).

  metric, mse_deviation   plain torch with the reference's return types: the generic route, and the cross-check of the one-launch scoring
                          (wdno_amd.burgers.score), which eval_ddpm_burgers.diffuse_2dconv takes for a BurgersMetric
  get_target              the reference re-reads and re-slices the test file on every call, five times per evaluation batch; here a file
                          is read once per (path, mtime), kept on the GPU, and its preprocessed view once per up-sampling level. The
                          wavelet branches run wdno_amd.wavelets (DWT1DForward, DWTForward) and wave_trans.coef_to_tensor
  load_2dconv_super_model out of scope (NotImplementedError, test_util.py:235-264): the cascade has no evaluation route here

Anything else falls through to the reference's module when that is on sys.path behind this tree."""
import os

import torch
from torch import nn

import wdno_amd

_reference_getattr = wdno_amd.reference_fallthrough('ddpm_burgers.test_util', __file__)

SOLVER_N_UPSAMPLE = 4          # precision of the solver: 2**4 = 16 grid points per field column


def mse_deviation(u1, u2, report_all=False):
    """Per-sample mean squared deviation over the last two axes (test_util.py:23-30); with report_all also the mean absolute deviation and
    both divided by the batch-wide mean of (u2 + 1e-5) squared / in absolute value."""
    d = u1 - u2
    if report_all:
        mse, mae, ep = d.square().mean((-1, -2)), d.abs().mean((-1, -2)), 1e-5
        return mse, mae, mse / (u2 + ep).square().mean(), mae / (u2 + ep).abs().mean()
    return d.square().mean((-1, -2))


def metric(u_target, f, total_upsample_t, wf=0, upsample_t=0, f_upsampled=None, report_all=False, u=None, evaluate=False):
    """The control metrics of test_util.py:33-98. u_target [B, Nt, Nx], f [B, Nt - 1, nx] (not rescaled). evaluate=True scores the given
    state u; otherwise the state is re-simulated from u_target[:, 0] under f. Returns (J_actual, control_energy, total_J) with J_actual the
    per-sample mse at the final time, or with report_all the tuple (mse, mse_median, mae, mae_median, nmse, nmae). As in the reference,
    nmse / nmae are normalised by a mean over the whole batch, and nmae is the square root of the mean absolute error over that."""
    from ddpm_burgers.generate_burgers import burgers_numeric_solve_free
    assert len(u_target.size()) == len(f.size()) == 3
    if evaluate:
        u_controlled = u
    elif f_upsampled is None:
        u_controlled = burgers_numeric_solve_free(u_target[:, 0], f, visc=0.01, T=8.0, num_t=80 * 2 ** upsample_t)
    else:
        u_controlled = burgers_numeric_solve_free(u_target[:, 0], f_upsampled[..., ::2], visc=0.01, T=8.0, num_t=160)[:, ::2]
    sub_N = int(u_controlled.shape[-1] / f.shape[-1])
    d = u_controlled[:, -1, :] - u_target[:, -1, :]
    t = u_target[:, -1, :]
    mse = d[:, ::sub_N].square().mean(-1)
    if report_all:
        ep = 1e-5
        J_actual = (mse, d.square().median(-1)[0], d.abs().mean(-1), d.abs().median(-1)[0],
                    d.square().mean(-1).sqrt() / (t.square().mean().sqrt() + ep), d.abs().mean(-1).sqrt() / (t.abs().mean().sqrt() + ep))
    else:
        J_actual = mse
    control_energy = f.square().sum((-1, -2)) / (2 ** upsample_t) ** 2
    return J_actual, control_energy, mse + wf * control_energy


def ddpm_guidance_loss(u_target, u, f, wu=0, wf=0, condition_f=False):
    """The control objective of test_util.py:100-126: wu (sum_b mean_x[(u0 - u0_gt)^2 (+ (uT - uT_gt)^2)] + wf sum f^2)."""
    loss_u = (u[:, 0, :] - u_target[:, 0, :]).square()
    if not condition_f:
        loss_u = loss_u + (u[:, -1, :] - u_target[:, -1, :]).square()
    return (loss_u.mean(-1).sum() + f.square().sum() * wf) * wu


# ------------------------------------------------------------------------------------------------ data sets and models
def load_burgers_dataset(args, RESCALER):
    from ddpm_burgers.data_burgers_1d import DiffusionDataset, get_burgers_preprocess
    return DiffusionDataset(f'data/{args.dataset}/train', preprocess=get_burgers_preprocess(rescaler=RESCALER))


def load_burgers_dataset_wavelet(args, RESCALER):
    from ddpm_burgers.data_burgers_1d import DiffusionDataset, get_wavelet_super_preprocess
    return DiffusionDataset(f'data/{args.dataset}/coef_{args.wave_type}_{args.pad_mode}_super',
                            preprocess=get_wavelet_super_preprocess(rescaler=1., is_super_model=False, mode=args.pad_mode, wave_type=args.wave_type,
                                                                    is_condition_u0=args.is_condition_u0, is_condition_uT=args.is_condition_uT))


_files = {}          # path -> (mtime, the file's dictionary with its tensors on the GPU)
_views = {}          # (path, mtime, device, N_upsample, dataset_kwargs) -> DiffusionDataset


def _test_dataset(path, N_upsample, device, dataset_kwargs):
    from ddpm_burgers.data_burgers_1d import DiffusionDataset, get_burgers_preprocess
    mtime = os.path.getmtime(path)
    dev = torch.device('cuda', device) if isinstance(device, int) else torch.device(device)
    key = (os.path.abspath(path), mtime, str(dev), int(N_upsample), tuple(sorted(dataset_kwargs.items())))
    ds = _views.get(key)
    if ds is None:
        held = _files.get(key[0])
        if held is None or held[0] != mtime or held[2] != str(dev):
            db = torch.load(path, weights_only=False)
            held = _files[key[0]] = (mtime, {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in db.items()}, str(dev))
            for k in [k for k in _views if k[0] == key[0] and k[1] != mtime]:
                del _views[k]
        ds = _views[key] = DiffusionDataset(held[1], preprocess=get_burgers_preprocess(rescaler=1., is_super_model_test=True, upsample_t=N_upsample,
                                                                                       upsample_x=N_upsample, **dataset_kwargs))
    return ds


def get_target(args, is_wave, target_i, f=False, N_upsample=0, device=0, dataset='free_u_f_1e5', **dataset_kwargs):
    """The evaluation targets of test_util.py:156-208 from data/{args.dataset}_super/test, not rescaled, on the GPU:
      is_wave=False          u (or f) [n, 81 2^N, 128 2^N] (rows not padded, columns padded)
      is_wave=True, f=False  the condition channel [n, 64 2^N, 64 2^N]: the 1-D DWT of u(t=0) and u(t=T) in four stripes
      is_wave=True, f=True   the packed 2-D DWT of f [n, 4, 64 2^N, 64 2^N]
    The returned tensors are fresh; the file is read once per path and modification time."""
    from wdno_amd import wavelets as W
    from wave_trans import coef_to_tensor
    ds = _test_dataset(f'data/{args.dataset}_super/test', N_upsample, device, dataset_kwargs)
    ori_shape = ds.ori_shape
    ret = ds.get(target_i)
    if ret.dim() == 3:                      # target_i an int
        ret = ret.unsqueeze(0)
    ret = ret[:, 1 if f else 0, :ori_shape[-2]]
    if not is_wave:
        return ret.clone()
    pad = 64 * 2 ** N_upsample
    if not f:
        lo, hi = W.DWT1DForward(J=1, mode=args.pad_mode, wave=args.wave_type)(ret[:, [0, -1], :ori_shape[-1]].contiguous())
        nx, n_repeat = lo.shape[-1], pad // 4
        cond = torch.zeros((ret.shape[0], pad, pad), device=ret.device)
        if args.is_condition_u0:
            cond[:, :n_repeat, :nx] = lo[:, [0]]
            cond[:, n_repeat:2 * n_repeat, :nx] = hi[0][:, [0]]
        if args.is_condition_uT:
            cond[:, 2 * n_repeat:3 * n_repeat, :nx] = lo[:, [1]]
            cond[:, 3 * n_repeat:4 * n_repeat, :nx] = hi[0][:, [1]]
        return cond
    yl, yh = W.DWTForward(J=1, mode=args.pad_mode, wave=args.wave_type)(ret[:, :, :ori_shape[-1]].unsqueeze(1).contiguous())
    ret = coef_to_tensor(yl, yh)[:, 0]
    return nn.functional.pad(ret, (0, pad - ret.shape[-1], 0, pad - ret.shape[-2]), 'constant', 0)


def get_2d_ddpm(shape, ori_shape, args, RESCALER, is_super_model, upsample_t=0, upsample_x=0):
    """The constructor mapping of train_ddpm_burgers.py:128-182 on this tree's Unet2D / GaussianDiffusion."""
    from ddpm_burgers.diffusion_1d import GaussianDiffusion
    from ddpm_burgers.unet import Unet2D
    side = 64 if args.is_wavelet else 128
    if args.is_wavelet:
        channels = 8 + (8 if is_super_model else 0) + (1 if args.is_condition_u0 or args.is_condition_uT else 0)
    else:
        channels = 4 if is_super_model else 2
    u_net = Unet2D(dim=args.dim, init_dim=None, out_dim=channels, dim_mults=args.dim_muls, channels=channels,
                   resnet_block_groups=args.resnet_block_groups)
    return GaussianDiffusion(
        u_net, seq_length=(side * 2 ** upsample_t, side * 2 ** upsample_x),
        is_wavelet=args.is_wavelet, padded_shape=shape, ori_shape=ori_shape, pad_mode=args.pad_mode, wave_type=args.wave_type,
        is_super_model=is_super_model, upsample_t=upsample_t, upsample_x=upsample_x,
        timesteps=args.timesteps, sampling_timesteps=args.ddim_sampling_steps if args.using_ddim else 1000, ddim_sampling_eta=args.ddim_eta,
        beta_schedule=args.beta_schedule, loss_layer_weight=RESCALER,
        is_condition_pad=args.is_condition_pad, is_condition_u0=args.is_condition_u0, is_condition_uT=args.is_condition_uT,
        is_condition_f=args.is_condition_f)


def load_2dconv_base_model(model_i, args, RESCALER):
    """The base model of test_util.py:212-233: the data set gives the shapes, a Trainer loads the checkpoint into the model."""
    from ddpm_burgers.train_diffusion import Trainer
    dataset = load_burgers_dataset_wavelet(args, RESCALER) if args.is_wavelet else load_burgers_dataset(args, RESCALER)
    ddpm = get_2d_ddpm(dataset.shape, dataset.ori_shape, args, RESCALER, is_super_model=False, upsample_t=0, upsample_x=0)
    trainer = Trainer(ddpm, dataset, is_super_model=False, wave_type=args.wave_type, pad_mode=args.pad_mode, rescaler=RESCALER,
                      results_folder=os.path.join(args.results_folder, model_i), train_num_steps=args.train_num_steps,
                      save_and_sample_every=args.checkpoint_interval)
    trainer.load(args.checkpoint if 'checkpoint' in args.__dict__ else 10)
    return ddpm


def load_2dconv_super_model(model_i, args, RESCALER):
    raise NotImplementedError('wdno_amd burgers evaluation: the super-resolution model is not provided here '
                              '(reference burgers/ddpm_burgers/test_util.py:235-264)')


def __getattr__(name):          # anything else of the reference module
    return _reference_getattr(name)
