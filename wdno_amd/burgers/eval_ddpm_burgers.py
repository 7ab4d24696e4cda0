"""MI355X drop-in for burgers/eval_ddpm_burgers.py: the driver that turns a Burgers checkpoint into the control table (J_actual, energy,
total_J, six metrics each for the diffused and the re-simulated state).

Same public names, signatures and command line as the reference: the parser (build_parser(); `parser`), get_loss_fn_2dconv,
get_nablaJ_2dconv, diffuse_2dconv, evaluate, save_eval_results and the __main__ block with the RESCALER table and the wfs x wus loop. With
this tree ahead of the reference on sys.path, `python eval_ddpm_burgers.py --exp_id ... --wus ... --wfs ...` runs the wavelet base model
end to end in one process:

  get_nablaJ_2dconv   wdno_amd.burgers.guidance.BurgersGuidance on the target get_target returns: the guided step is the fused,
                      graph-replayed one
  diffuse_2dconv      sample(), then wdno_amd.burgers.reconstruct.reconstruct: one launch (csrc/burgers_reconstruct.hip); the solver
                      (csrc/burgers.hip) writing only the columns the metrics read; then, for a BurgersMetric, wdno_amd.burgers.score.score:
                      one launch (csrc/burgers_score.hip) and one device-to-host copy. Any other custom_metric is called exactly as the
                      reference calls it, on the reconstructed tensors
  evaluate            the reference's seeding, batching and nested result list; the test file is read once (test_util.get_target) and ONE
                      BurgersGuidance per batch size is moved from target to target with set_target, so the captured sampling step --
                      keyed on the object's identity -- is replayed on every batch instead of being captured again
  save_eval_results   the reference's 15 YAML entries per resolution through result_io.save_acc

and, with `--is_super_model True --upsample_t k --upsample_x k --super_exp_id ...` (two checkpoints), the zero-shot super-resolution cascade
of l.254-258, 306-338 after every base batch:

  evaluate            per level k = 1 .. upsample_x one launch (wdno_amd.burgers.cascade.super_conditions, csrc/burgers_cascade.hip) writes
                      the super model's whole condition source from the previous level's block and two rows of the level's target, read
                      in place from the held test file (wdno_amd.burgers.cascade.get_target_view); the level samples unguided (the reference's wu = wf = 0)
  diffuse_2dconv      N_upsample=k takes entry k - 1 of the model's shape lists; cond_src= (an extension) goes to sample_with_source; the
                      reconstruction reads channels 0-7 of the 17-channel sample; the solver runs 80 2^k records on the level's forcing

Out of scope, raising NotImplementedError with the reference's line: is_wavelet=False (eval_ddpm_burgers.py:126-132, 180-182, 196-197);
is_super_model=True with upsample_x=0 (:307, a cascade without a level to run); N_upsample / low without args.is_super_model (:175-178);
is_super_model together with is_condition_f, the three-way interpolation MSE (:207-218). Anything else falls through to the reference's
module when that is on sys.path behind this tree."""
import argparse
import math

import numpy as np
import torch

import wdno_amd
from ddpm_burgers.generate_burgers import burgers_numeric_solve_free          # looked up as a module global at call time
from ddpm_burgers.model_utils import get_scheduler
from ddpm_burgers.test_util import (SOLVER_N_UPSAMPLE, ddpm_guidance_loss, get_target, load_2dconv_base_model,  # noqa: F401
                                    metric, mse_deviation)
from wdno_amd.burgers.cascade import get_target_view, load_super_model as load_2dconv_super_model      # ddpm_burgers.test_util's still refuses
from result_io import save_acc          # this tree's top-level module (see its docstring)

_reference_getattr = wdno_amd.reference_fallthrough('eval_ddpm_burgers', __file__)


def _unsupported(what, line):
    raise NotImplementedError(f'wdno_amd burgers evaluation: {what} is not provided here (reference burgers/eval_ddpm_burgers.py:{line})')


def build_parser():
    """The reference's argument parser (eval_ddpm_burgers.py:21-103): the same options, types and defaults."""
    p = argparse.ArgumentParser(description='Eval EBM model')
    for name, kw in (
            ('--exp_id', dict(type=str)), ('--super_exp_id', dict(default='', type=str)), ('--results_folder', dict(default='./results/', type=str)),
            ('--save_file', dict(default='results/evaluate/result.yaml', type=str)), ('--dataset', dict(default='1d', type=str)),
            ('--model_str', dict(default='', type=str)), ('--report_all', dict(default=True, type=eval)),
            ('--Ntest', dict(default=50, type=int)), ('--batch_size', dict(default=50, type=int)),
            ('--upsample_t', dict(default=0, type=int)), ('--upsample_x', dict(default=0, type=int)),
            ('--is_wavelet', dict(default=True, type=eval)), ('--is_super_model', dict(default=False, type=eval)),
            ('--wave_type', dict(default='bior2.4', type=str)), ('--pad_mode', dict(default='periodization', type=str)),
            ('--checkpoint', dict(default=10, type=int)), ('--super_checkpoint', dict(default=10, type=int)),
            ('--checkpoint_interval', dict(default=10000, type=int)), ('--train_num_steps', dict(default=100000, type=int)),
            ('--using_ddim', dict(default=False, type=eval)), ('--ddim_eta', dict(default=0., type=float)),
            ('--ddim_sampling_steps', dict(default=100, type=int)), ('--J_scheduler', dict(default=None, type=str)),
            ('--wfs', dict(nargs='+', default=[0], type=float)), ('--wus', dict(nargs='+', default=[0], type=float)),
            ('--timesteps', dict(default=1000, type=int)), ('--beta_schedule', dict(default='cosine', type=str)),
            ('--is_condition_pad', dict(default=True, type=eval)), ('--is_condition_u0', dict(default=False, type=eval)),
            ('--is_condition_uT', dict(default=False, type=eval)), ('--is_condition_f', dict(default=False, type=eval)),
            ('--dim', dict(default=128, type=int)), ('--resnet_block_groups', dict(default=1, type=int)),
            ('--dim_muls', dict(nargs='+', default=[1, 2, 4, 8], type=int)), ('--super_dim', dict(default=64, type=int))):
        p.add_argument(name, **kw)
    return p


parser = build_parser()


# ------------------------------------------------------------------------------------------------ loss, guidance and metric
def get_loss_fn_2dconv(args, shape, ori_shape, RESCALER, is_super_model=False, low=0, N_upsample=0, wf=0, wu=0, target_i=0, device=0, dataset='1d',
                       condition_f=False):
    """The differentiable control objective of the targets target_i (eval_ddpm_burgers.py:108-144) on wdno_amd.wavelets.DWTInverse."""
    from wdno_amd.burgers.guidance import guidance_value
    if not args.is_wavelet:
        _unsupported('is_wavelet=False', '126-132')
    u_target = get_target(args, is_wave=False, target_i=target_i, N_upsample=N_upsample, device=device, dataset=dataset)
    return lambda x: guidance_value(x, u_target, shape, ori_shape, torch.as_tensor(RESCALER).to(x.device), wu, wf, condition_f, args.wave_type,
                                    args.pad_mode, is_super_model)


def get_nablaJ_2dconv(**kwargs):
    """nablaJ for GaussianDiffusion.sample, with get_loss_fn_2dconv's keywords: a BurgersGuidance (closed form, one launch, graph-safe) on
    the target rows of target_i; configurations its kernel does not take differentiate the objective above inside the object."""
    from wdno_amd.burgers.guidance import BurgersGuidance
    args = kwargs['args']
    if not args.is_wavelet:
        _unsupported('is_wavelet=False', '126-132')
    u_target = get_target(args, is_wave=False, target_i=kwargs.get('target_i', 0), N_upsample=kwargs.get('N_upsample', 0),
                          device=kwargs.get('device', 0), dataset=kwargs.get('dataset', '1d'))
    return BurgersGuidance(kwargs['shape'], kwargs['ori_shape'], kwargs['RESCALER'], u_target, kwargs.get('wu', 0), kwargs.get('wf', 0),
                           condition_f=kwargs.get('condition_f', False), wave_type=args.wave_type, pad_mode=args.pad_mode,
                           is_super_model=kwargs.get('is_super_model', False))


class BurgersMetric:
    """custom_metric of diffuse_2dconv with metric()'s keyword signature: called, it is
    metric(u_target_ori, f, total_upsample_t, wf=wf, report_all=report_all, **kwargs); seen by diffuse_2dconv on the wavelet model, it
    selects the one-launch scoring (wdno_amd.burgers.score) of the same numbers."""

    def __init__(self, u_target_ori, total_upsample_t, wf, report_all):
        self.u_target, self.total_upsample_t, self.wf, self.report_all = u_target_ori, total_upsample_t, wf, report_all

    def __call__(self, f, **kwargs):
        return metric(self.u_target, f, self.total_upsample_t, wf=self.wf, report_all=self.report_all, **kwargs)


# ------------------------------------------------------------------------------------------------ one batch
def diffuse_2dconv(ddpm, args, custom_metric, ret_ls=False, RESCALER=1, **kwargs):
    """Samples from the diffusion model and scores the result (eval_ddpm_burgers.py:152-242). Returns the reference's 6-tuple:
    x [B, 8, h, w] (the rescaled coefficient block), ddpm_mse (CPU tensor [B]), J_diffused, J_actual ((6, B) numpy arrays with report_all,
    else (B,)), energy [B], total_J [B]. With a BurgersMetric the arrays and ddpm_mse are float64 (formed in fp64 from the fp32 fields)
    where the reference has float32; any other custom_metric gives what it returns, converted as the reference converts it."""
    from wdno_amd.burgers.reconstruct import reconstruct
    from wdno_amd.burgers import score as S
    is_super = bool(getattr(args, 'is_super_model', False))
    if ('N_upsample' in kwargs or 'low' in kwargs) and not is_super:
        _unsupported('N_upsample / low without args.is_super_model', '175-178, 189-190')
    if is_super and getattr(args, 'is_condition_f', False):
        _unsupported('is_super_model=True with is_condition_f=True (the three-way interpolation MSE)', '207-218')
    if not ddpm.is_wavelet or not getattr(args, 'is_wavelet', True):
        _unsupported('is_wavelet=False', '180-182, 196-197')
    cond_src = kwargs.pop('cond_src', None)          # an extension: the super level's condition source, assembled (burgers/cascade.py)
    if 'N_upsample' not in kwargs:
        shape, ori_shape, N_upsample = ddpm.padded_shape, ddpm.ori_shape, 0
    else:
        N_upsample = int(kwargs['N_upsample'])
        shape, ori_shape = ddpm.padded_shape[N_upsample - 1], ddpm.ori_shape[N_upsample - 1]
    h, w, n_x = int(shape[-2]), int(shape[-1]), int(ori_shape[-1])

    sample = ddpm.sample(**kwargs) if cond_src is None else ddpm.sample_with_source(cond_src, **kwargs)
    u, f = reconstruct(sample, shape, ori_shape, RESCALER, args.wave_type, args.pad_mode)
    r = torch.as_tensor(RESCALER, dtype=torch.float32).reshape(-1).to(sample.device)
    x = sample[:, :8, :h, :w] * (r if r.numel() == 1 else r[:8].reshape(1, 8, 1, 1))

    if ddpm.is_condition_f:
        x_gt = kwargs['x_gt'][:, :, :n_x * 2 ** (args.upsample_x - N_upsample)]
    elif args.upsample_x == 0:
        # the reference solves at 1920 points and keeps [:, :, ::16]; the solver's own down-sampling is that slice (sub_s = int(1920 / 120))
        x_gt = burgers_numeric_solve_free(u[:, 0], f, visc=0.01, T=8.0, num_t=80 * 2 ** N_upsample, output_space_downsample=True)
    else:
        x_gt = burgers_numeric_solve_free(u[:, 0], f, visc=0.01, T=8.0, num_t=80 * 2 ** N_upsample, output_space_downsample=False)\
            [:, :, ::2 ** (SOLVER_N_UPSAMPLE - args.upsample_x)]

    if isinstance(custom_metric, BurgersMetric):
        ut = torch.as_tensor(custom_metric.u_target).to(u.device, torch.float32)
        if ut.shape[1] != u.shape[1]:
            ut = ut[:, -1:].expand(ut.shape[0], u.shape[1], ut.shape[2])          # only the last row is read
        ddpm_mse, J_diffused, J_actual, energy, total_J = S.score(u, f, x_gt.to(torch.float32), ut, custom_metric.wf, upsample_t=N_upsample,
                                                                  report_all=custom_metric.report_all, actual_is_diffused=bool(ddpm.is_condition_f))
        return x, torch.from_numpy(ddpm_mse), J_diffused, J_actual, energy, total_J

    sub_N = int(x_gt.shape[-1] / u.shape[-1])
    ddpm_mse = mse_deviation(u[:, 1:], x_gt[:, 1:, ::sub_N]).cpu()
    u_repeat = u.unsqueeze(-1).expand(u.shape[0], u.shape[1], u.shape[2], sub_N).reshape(u.shape[0], u.shape[1], u.shape[2] * sub_N)[:, :, :x_gt.shape[2]]
    J_diffused, _, _ = custom_metric(f, upsample_t=N_upsample, u=u_repeat, evaluate=True)
    J_actual, energy, total_J = custom_metric(f, upsample_t=N_upsample, u=u_repeat if ddpm.is_condition_f else x_gt, evaluate=True)
    to_numpy = lambda v: v.detach().cpu().numpy() if type(v) is not tuple else np.array([vi.detach().cpu().numpy() for vi in v])
    return x, ddpm_mse, to_numpy(J_diffused), to_numpy(J_actual), energy.detach().cpu().numpy(), total_J.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ the whole test set
def evaluate(model_i, super_model_i, args, Ntest=50, batch_size=25, wu=0, wf=0, RESCALER=1):
    """The evaluation of eval_ddpm_burgers.py:244-344: per resolution k = 0 .. upsample_x (0 alone without is_super_model) the list
    [ddpm_mse, the J_diffused rows, the J_actual rows, energy, total_J], every entry an array over the Ntest samples.

    With is_super_model the zero-shot cascade of l.306-338 follows every base batch: per level one launch (burgers/cascade.py:
    super_conditions) turns the previous level's returned block and two rows of the level's target -- a strided view of the held test file
    -- into the super model's condition source, which diffuse_2dconv hands to sample_with_source. The super levels sample unguided, through
    the graph-replayed loop: the reference passes wu = wf = 0 there (l.331), so its guidance adds an identically zero gradient; nor is f
    transformed at those levels (the sampler reads it only under is_condition_f, which is out of scope with a super model)."""
    if not args.is_wavelet:
        _unsupported('is_wavelet=False', '126-132, 180-182, 196-197')
    if args.is_super_model:                     # refusals before anything is loaded
        if args.upsample_x < 1:
            _unsupported('is_super_model=True with upsample_x=0 (a cascade without a super level)', '307')
        if args.is_condition_f:
            _unsupported('is_super_model=True with is_condition_f=True (the three-way interpolation MSE)', '207-218')
    ddpm = load_2dconv_base_model(model_i, args, RESCALER)
    levels = 0
    if args.is_super_model:
        from wdno_amd.burgers import cascade as CS
        ddpm_super = load_2dconv_super_model(super_model_i, args, RESCALER)
        levels = args.upsample_x
    RESCALER = torch.as_tensor(RESCALER).cuda()
    RESCALER_base = RESCALER[:, 8:17] if args.is_super_model else RESCALER
    rescaler_f32 = RESCALER.to(torch.float32).reshape(-1).contiguous()          # the table is int64: cast once, not in every hand-off
    rep = math.ceil(Ntest / batch_size)
    logs = {k: {'mses': [], 'l_gts': [], 'l_dfs': [], 'energies': [], 'l_total': []} for k in range(levels + 1)}
    sampled_coefs = []
    guidance = {}                          # batch size -> the BurgersGuidance whose captured step serves every batch of that size

    for i in range(rep):
        print("Batch No.", i)
        torch.manual_seed(i)
        torch.cuda.manual_seed(0)
        if (i + 1) * batch_size <= Ntest:
            target_idx = list(range(i * batch_size, (i + 1) * batch_size))
        else:
            target_idx = list(range(i * batch_size, Ntest))
            batch_size = Ntest - i * batch_size

        u_target_ori = get_target(args, is_wave=False, target_i=target_idx, N_upsample=args.upsample_x, dataset=args.dataset)\
            [:, :, :ddpm.ori_shape[-1] * 2 ** args.upsample_x]
        u_condition = get_target(args, is_wave=True, target_i=target_idx, dataset=args.dataset)
        nablaJ = guidance.get(batch_size)
        if nablaJ is None:
            nablaJ = guidance[batch_size] = get_nablaJ_2dconv(args=args, shape=ddpm.padded_shape, ori_shape=ddpm.ori_shape, RESCALER=RESCALER_base,
                                                              target_i=target_idx, wu=wu, wf=wf, dataset=args.dataset, condition_f=args.is_condition_f)
        else:
            nablaJ.set_target(get_target(args, is_wave=False, target_i=target_idx, dataset=args.dataset))

        sampled_coef, ddpm_mse, J_diffused, J_actual, energy, total_J = diffuse_2dconv(
            ddpm, args, RESCALER=RESCALER_base, batch_size=batch_size,
            J_scheduler=get_scheduler(args.J_scheduler),
            custom_metric=BurgersMetric(u_target_ori, args.upsample_t, wf, args.report_all),
            u_init=u_condition[:, :32] / RESCALER_base.squeeze()[-1],
            u_final=u_condition[:, -32:] / RESCALER_base.squeeze()[-1],
            f=get_target(args, f=True, is_wave=True, target_i=target_idx, dataset=args.dataset) / RESCALER_base[:, 4:8],
            x_gt=u_target_ori,
            nablaJ=nablaJ,
        )
        logs[0]['mses'].append(ddpm_mse)
        logs[0]['l_gts'].append(J_actual)
        logs[0]['l_dfs'].append(J_diffused)
        logs[0]['energies'].append(energy)
        logs[0]['l_total'].append(total_J)
        sampled_coefs.append(sampled_coef.cpu().numpy())

        for k in range(1, levels + 1):          # zero-shot super-resolution (l.306-338)
            pad_size = 64 * 2 ** k
            src = CS.super_conditions(sampled_coef, get_target_view(args, target_idx, N_upsample=k, dataset=args.dataset), rescaler_f32,
                                      ddpm_super.padded_shape[k - 1], pad_size, pad_size, args.is_condition_u0, args.is_condition_uT,
                                      args.wave_type, args.pad_mode)
            low, u_init, u_final = CS.views(src)
            sampled_coef, ddpm_mse, J_diffused, J_actual, energy, total_J = diffuse_2dconv(
                ddpm_super, args, N_upsample=k, RESCALER=RESCALER, batch_size=batch_size,
                J_scheduler=get_scheduler(args.J_scheduler),
                custom_metric=BurgersMetric(u_target_ori, args.upsample_t, wf, args.report_all),
                cond_src=src, low=low, u_init=u_init, u_final=u_final,
                x_gt=u_target_ori,
            )
            logs[k]['mses'].append(ddpm_mse)
            logs[k]['l_gts'].append(J_actual)
            logs[k]['l_dfs'].append(J_diffused)
            logs[k]['energies'].append(energy)
            logs[k]['l_total'].append(total_J)

    return [[np.concatenate(logs[k]['mses']),
             *(np.concatenate(logs[k]['l_dfs'], axis=1)[i] for i in range(logs[k]['l_dfs'][0].shape[0])),
             *(np.concatenate(logs[k]['l_gts'], axis=1)[i] for i in range(logs[k]['l_dfs'][0].shape[0])),
             np.concatenate(logs[k]['energies']),
             np.concatenate(logs[k]['l_total'])] for k in range(args.upsample_x + 1) if k in logs]


def result_names(k, attr=''):
    """The 15 entry names of resolution k, in the order of evaluate()'s list (eval_ddpm_burgers.py:351-357)."""
    return [f'mse_gt_{k}_{attr}, linear sr/nearest sr/without sr:',
            f'J_diffused_mse_{k}_{attr}', f'J_diffused_mse_median_{k}_{attr}', f'J_diffused_mae_{k}_{attr}', f'J_diffused_mae_median_{k}_{attr}',
            f'J_diffused_nmse_{k}_{attr}', f'J_diffused_nmae_{k}_{attr}', f'J_actual_mse_{k}_{attr}', f'J_actual_mse_median_{k}_{attr}',
            f'J_actual_mae_{k}_{attr}', f'J_actual_mae_median_{k}_{attr}', f'J_actual_nmse_{k}_{attr}', f'J_actual_nmae_{k}_{attr}',
            f'energy_{k}_{attr}', f'totalJ_{k}_{attr}']


def save_eval_results(save_values, model_i, fname, model_str='', wu=None, wf=None):
    """mean / std of every entry into the YAML file fname under {model_i: {'model_description', 'wu=.., wf=..': {name: ...}}}. The
    reference reads wu and wf from the enclosing __main__ loop; they may be passed here, and default to this module's globals."""
    wu = globals().get('wu', 0) if wu is None else wu
    wf = globals().get('wf', 0) if wf is None else wf
    print('Evaluated on super, current and base resolution。')
    for k in range(len(save_values)):
        for acc, inner_str in zip(save_values[k], result_names(k)):
            print(k, inner_str, acc.mean(0))
            save_acc(acc, fname,
                     make_dict_path=lambda acc, dict_args, inner_str=inner_str: {
                         dict_args['model_name']: {'model_description': dict_args['model_str'], dict_args['guidance_str']: {inner_str: acc}}},
                     model_name=f'{model_i}', model_str=model_str, guidance_str=f'wu={wu:.1f}, wf={wf:.1f}')


def rescaler_table(args):
    """The RESCALER of the __main__ block (eval_ddpm_burgers.py:386-405)."""
    if not args.is_wavelet:
        return torch.tensor([10])
    table = {'bior2.4': [10, 3, 3, 1, 21, 5, 5, 1], 'bior1.3': [8, 5, 4, 2, 21, 4, 3, 1], 'db4': [8, 4, 3, 2, 21, 3, 3, 1], 'sym4': [8, 5, 4, 2, 21, 6, 6, 2]}
    if args.pad_mode != 'periodization' or args.wave_type not in table:
        raise ValueError('Input RESCALER.')
    RESCALER = torch.tensor(table[args.wave_type]).view(1, 8, 1, 1)
    if args.is_super_model:
        RESCALER = RESCALER.repeat(1, 2, 1, 1)
    if args.is_condition_u0 or args.is_condition_uT:
        RESCALER = torch.cat((RESCALER, 10 * torch.ones_like(RESCALER[:, [0]])), dim=1)
    return RESCALER


def __getattr__(name):          # anything else of the reference module
    return _reference_getattr(name)


if __name__ == '__main__':
    args = parser.parse_args()
    if args.is_super_model:
        assert args.upsample_t == args.upsample_x, "super model only support the same upsample_t and upsample_x"
    model_i, super_model_i, cp, super_cp, model_str = args.exp_id, args.super_exp_id, args.checkpoint, args.super_checkpoint, args.model_str
    RESCALER = rescaler_table(args)
    print(args)
    print('Results saved in: ', args.save_file)
    for wf in args.wfs:
        for wu in args.wus:
            print(f'wu={wu:.2f}, wf={wf:.7f}')
            results = evaluate(model_i=model_i, super_model_i=super_model_i, args=args, Ntest=args.Ntest, batch_size=args.batch_size, wu=wu, wf=wf,
                               RESCALER=RESCALER)
            save_eval_results(results,
                              model_i=model_i + super_model_i + ' checkpoint=' + str(cp) + ' super checkpoint=' + str(super_cp)
                              + ' ddim_sampling_steps=' + str(args.ddim_sampling_steps) + ' ddim_eta=' + str(args.ddim_eta),
                              fname=args.save_file, model_str=model_str + f'u0 guidance, rescaler {RESCALER.squeeze()}')
