"""MI355X drop-in for smoke/inference_2d.py: the driver that turns a test batch into conditions, samples, rebuilds the fields and scores them.

Same public names and signatures as the reference: guidance_fn, load_model, InferencePipeline (run_base_model, run_super_model, run_model,
run, save_results, per_evaluate, multi_evaluate_control, multi_evaluate), inference, main, and the argument parser under __main__. With this
tree ahead of the reference on sys.path, `python inference_2d.py --is_wavelet True ...` runs the wavelet base model end to end:

  load_model              design_fn = wdno_amd.smoke.guidance.SmokeGuidance: the guided step is the fused, graph-replayed one
  run_model               the conditions from the launches of ddpm.data_2d.pack_smoke_fields on the five fields of the base-resolution state
                          (one permuting copy), zero curve: channel C - 2 is wave_init / RESCALER[-2] with each sub-band shown for
                          pad_t / 4 frames, channels 24:40 are wave_control / RESCALER[24:40]
  run_base_model          sample(), then wdno_amd.smoke.reconstruct.reconstruct: one launch (csrc/smoke_reconstruct.hip)
  multi_evaluate_control  the reference's contract through wdno_amd.smoke_solver.evaluate_controls: one process, one launch, no fork
  multi_evaluate          the reference's five arrays through wdno_amd.smoke.score: score_controls (the solver writes only the frames the
                          metrics read; csrc/smoke_score.hip reads them in place) or score (simulation mode)
  run / save_results      the reference's results.txt / results_sim.txt lines

and, with `--is_super_model True --upsample 1 --is_condition_control True`, the zero-shot space super-resolution cascade (a model list of two):

  load_model              the base model on RESCALER[:, :, 40:], the super model on RESCALER; design_fn = wdno_amd.smoke.guidance.CascadeGuidance,
                          a SmokeGuidance per level, so both levels keep the fused, graph-replayed guided step
  run_super_model         sample() of the base model; wdno_amd.smoke.cascade.super_conditions: low, init and control of the super level as the
                          sampler's condition source in two launches (csrc/smoke_cascade.hip), handed over by sample_with_source; sample() of
                          the super model; reconstruct() per level, the super level's block at offset 1 and its smoke-out rows split at 40
  multi_evaluate          per level the reference's four comparisons (base / current / linear / nearest) from one launch
                          (wdno_amd.smoke.score.score_super), mse_wo_smoke in the mse slot as in the reference (l.447-448)
  run                     scores every level into J_totals[i] ... n_l2s[i]

Out of scope, raising NotImplementedError with the reference's line: is_wavelet=False (inference_2d.py:133-136); is_super_model=True with
upsample=0 (a cascade without a super level is the base driver), a two-model list without is_super_model and run_super_model on a
one-model pipeline (inference_2d.py:155-232); upsample >= 2 (inference_2d.py:177: the slice step 2 ** (1 - i) is fractional there);
is_super_model=True with is_condition_control=False (inference_2d.py:157: the reference asserts it); plot=True (inference_2d.py:372-378).
Anything else falls through to the reference's module when that is on sys.path behind this tree."""
import argparse
import datetime
import os
import time

import numpy as np
import torch

import wdno_amd

_reference_getattr = wdno_amd.reference_fallthrough('inference_2d', __file__)

PAD_T, PAD_X = 24, 40          # run_model's hard-coded padded tensor (inference_2d.py:243)


def _unsupported(what, line):
    raise NotImplementedError(f'wdno_amd smoke inference: {what} is not provided here (reference smoke/inference_2d.py:{line})')


def guidance_fn(x, args, shape, ori_shape, RESCALER, w_energy=0, w_init=0, low=None, init=None, init_u=None):
    """dJ/d(x RESCALER) of the control objective (inference_2d.py:30-66), from the closed form of wdno_amd.smoke.guidance."""
    from wdno_amd.smoke import guidance as G
    if not args.is_wavelet:
        _unsupported('is_wavelet=False', '56-63')
    return G.guidance_fn_explicit(x, shape, ori_shape, RESCALER.to(x.device), args.wave_type, args.pad_mode, args.is_condition_control, w_energy,
                                  w_init, init_u)


def _check_cascade(args, line):
    """The one cascade the reference can run: upsample=1 in simulation mode."""
    up = int(getattr(args, 'upsample', 0))
    if up == 0:
        _unsupported('is_super_model=True with upsample=0 (a cascade without a super level is the base driver)', line)
    if up >= 2:
        _unsupported(f'upsample={up} (the reference slices the fields with the step 2 ** (1 - i), fractional for i >= 2; its data is 2x the base grid)', '177')
    if not args.is_condition_control:
        _unsupported('is_super_model=True with is_condition_control=False (the reference asserts is_condition_control)', '157')


def load_model(args, shape, ori_shape, RESCALER):
    if not args.is_wavelet:
        _unsupported('is_wavelet=False', '56-63')
    from wdno_amd.smoke.guidance import CascadeGuidance, SmokeGuidance
    if args.is_super_model:
        _check_cascade(args, '72-75')
        from ddpm.utils import load_ddpm_base_model, load_ddpm_super_model      # the reference's loaders, on this tree's model classes
        diffusion, device = load_ddpm_base_model(args, shape[0], ori_shape[0], RESCALER[:, :, 40:])
        diffusion_super, device = load_ddpm_super_model(args, shape, ori_shape, RESCALER)
        kw = dict(is_condition_control=args.is_condition_control, w_energy=args.w_energy, w_init=args.w_init, wave_type=args.wave_type,
                  pad_mode=args.pad_mode)
        levels = [SmokeGuidance(shape[0], ori_shape[0], RESCALER[:, :, 40:], **kw)]
        levels += [SmokeGuidance(shape[i], ori_shape[i], RESCALER, **kw) for i in range(1, int(args.upsample) + 1)]
        return [diffusion, diffusion_super], CascadeGuidance(levels)
    from ddpm.utils import load_ddpm_base_model          # the reference's loader (falls through ddpm/__init__.py), on this tree's model classes
    diffusion, device = load_ddpm_base_model(args, shape, ori_shape, RESCALER)
    design_fn = SmokeGuidance(shape, ori_shape, RESCALER, is_condition_control=args.is_condition_control, w_energy=args.w_energy,
                              w_init=args.w_init, wave_type=args.wave_type, pad_mode=args.pad_mode)
    return [diffusion], design_fn


class InferencePipeline(object):
    def __init__(self, model, args=None, RESCALER=1, results_path=None, args_general=None):
        super().__init__()
        self.model = model
        self.args = args
        self.results_path = results_path
        self.args_general = args_general
        self.is_wavelet = args_general.is_wavelet
        self.is_condition_control = args_general.is_condition_control
        self.image_size = self.args_general.image_size
        self.device = self.args_general.device
        self.upsample = args_general.upsample
        self.RESCALER = RESCALER
        if not self.is_wavelet:
            _unsupported('is_wavelet=False', '133-136')
        self.is_super_model = bool(getattr(args_general, 'is_super_model', False))
        if self.is_super_model:
            _check_cascade(args_general, '155-232')
        if len(model) != (2 if self.is_super_model else 1):
            _unsupported(f'a list of {len(model)} models with is_super_model={self.is_super_model}', '155-232')
        if not os.path.exists(self.results_path):
            os.makedirs(self.results_path)

    def run_base_model(self, state, wave_init, wave_control):
        """The reference's contract: state [B, to, 6, ho, wo] not rescaled, wave_init [B, pad_t, pad_x, pad_x] and wave_control
        [B, pad_t, 16, pad_x, pad_x] NOT yet divided by RESCALER. Returns pred [B, to, 6, ho, wo]."""
        r = torch.as_tensor(self.RESCALER).to(wave_init.device)
        return self._sample_and_reconstruct(state, wave_init / r[:, :, -2], wave_control / r[:, :, 24:40])

    def _sample_and_reconstruct(self, state, init, control):
        """sample() on conditions in network units, then the one-launch reconstruction."""
        from wdno_amd.smoke.reconstruct import reconstruct
        m = self.model[0]
        output = m.sample(batch_size=state.shape[0], design_fn=self.args['design_fn'], design_guidance=self.args['design_guidance'], low=None,
                          init=init, init_u=state[:, 0, 0], control=control)
        return reconstruct(output, m.padded_shape, m.ori_shape, self.RESCALER, m.wave_type, m.pad_mode)

    def run_super_model(self, state, state_ori, wave_init, wave_control):
        """The reference's contract: state [B, to, 6, ho, wo] the base-resolution state, state_ori [B, to, 6, 2 ho, 2 wo] the batch as loaded,
        wave_init / wave_control the base level's conditions NOT yet divided by RESCALER. Returns [pred_0, pred_1]."""
        if len(self.model) != 2:
            _unsupported('run_super_model on a one-model pipeline', '155-232')
        r = torch.as_tensor(self.RESCALER).to(wave_init.device)
        return self._cascade(state, state_ori, wave_init / r[:, :, -2], wave_control / r[:, :, 24:40])

    def _cascade(self, state, state_ori, init, control):
        """Base sample, the super level's conditions (network units throughout), super sample, one reconstruction per level."""
        from wdno_amd.smoke.cascade import super_conditions, views
        from wdno_amd.smoke.reconstruct import level_rescaler, reconstruct
        m0, m1 = self.model
        shape, ori_shape = m1.padded_shape, m1.ori_shape
        kw = dict(batch_size=state.shape[0], design_fn=self.args['design_fn'], design_guidance=self.args['design_guidance'])
        out0 = m0.sample(low=None, init=init, init_u=state[:, 0, 0], control=control, **kw)
        fine = state_ori.to(out0.device, torch.float32)          # level 1 of simulation mode: the batch at stride 2 ** (1 - 1) (l.177)
        pad_t, pad_x = int(getattr(m0, 'frames', PAD_T)), 2 * int(getattr(m0, 'image_size', PAD_X))
        src = super_conditions(out0, shape[0], fine, self.RESCALER, shape[1], pad_t, pad_x, m1.wave_type, m1.pad_mode)
        low, init1, control1 = views(src)
        kw1 = dict(N_upsample=1, low=low, init=init1, init_u=fine[:, 0, 0], control=control1, **kw)
        out1 = m1.sample_with_source(src, **kw1) if hasattr(m1, 'sample_with_source') else m1.sample(**kw1)
        preds = []
        for i, out in enumerate((out0, out1)):                    # l.213-231: both levels on the super model's RESCALER, rows split at int(H / 2)
            preds.append(reconstruct(out, shape[i], ori_shape[i], level_rescaler(self.RESCALER, out.shape[2]), m0.wave_type, m0.pad_mode,
                                     upsample_type='space' if i else None, half=int(out.shape[-2] / 2)))
        return preds

    def run_model(self, state):
        """state: not rescaled, [B, 256, 6, nx, nx] (control) or [B, nt, 6, 2 nx, 2 nx] (simulation)."""
        from ddpm.data_2d import pack_smoke_fields
        state_ori = state.to(self.device)
        state = state_ori[:, ::8] if not self.args_general.is_condition_control else state_ori[:, :, :, ::2, ::2]      # base resolution
        state = state.to(torch.float32)
        fields = state[:, :, :5].permute(0, 2, 1, 3, 4).contiguous()
        curve = torch.zeros(fields.shape[0], fields.shape[2], device=fields.device, dtype=torch.float32)
        m = self.model[0]               # the sampler's tensor: 24 frames of 40 x 40 in the reference, whatever the model says it is here
        resc = torch.as_tensor(self.RESCALER).reshape(-1)[-42:]      # the base level's 42 entries (RESCALER[:, :, 40:] of a super model's 82)
        packed = pack_smoke_fields(fields, curve, resc, wave=m.wave_type, pad_t=int(getattr(m, 'frames', PAD_T)),
                                   pad_x=int(getattr(m, 'image_size', PAD_X)))
        if len(self.model) == 2:
            return self._cascade(state, state_ori, packed[:, :, -2].contiguous(), packed[:, :, 24:40].contiguous())
        return self._sample_and_reconstruct(state, packed[:, :, -2].contiguous(), packed[:, :, 24:40].contiguous())

    def run(self, dataloader):
        preds = []
        J_totals, J_targets, J_energys, mses, n_l2s = {}, {}, {}, {}, {}
        for i in range(self.upsample + 1):
            J_totals[i], J_targets[i], J_energys[i], mses[i], n_l2s[i] = [], [], [], [], []
        for i, data in enumerate(dataloader):
            print(f"Batch No.{i}")
            state, shape, ori_shape, sim_id = data
            pred = self.run_model(state)
            preds.append(pred)
            for lvl, p in enumerate(pred if self.is_super_model else [pred]):
                if self.is_super_model:
                    print('Number of upsampling times:', lvl)
                J_total, J_target, J_energy, mse, n_l2 = self.multi_evaluate(p, state, plot=False)
                J_totals[lvl].append(J_total)
                J_targets[lvl].append(J_target)
                J_energys[lvl].append(J_energy)
                mses[lvl].append(mse)
                n_l2s[lvl].append(n_l2)
        print("Final results!")
        for i in range(self.upsample + 1):
            print(f"Number of upsampling times: {i}")
            print(self._lines(i, J_totals, J_targets, J_energys, mses, n_l2s))
        self.save_results(J_totals, J_targets, J_energys, mses, n_l2s)

    @staticmethod
    def _lines(i, J_totals, J_targets, J_energys, mses, n_l2s):
        return (f"J_total: {np.stack(J_totals[i]).mean(0)},\nJ_target: {np.stack(J_targets[i]).mean(0)},\nJ_energy: "
                f"{np.stack(J_energys[i]).mean(0)},\nmse: {np.stack(mses[i]).mean(0)},\nn_l2: {np.stack(n_l2s[i]).mean(0)}")

    def save_results(self, J_totals, J_targets, J_energys, mses, n_l2s):
        save_file = 'results_sim.txt' if self.args_general.is_condition_control else 'results.txt'
        with open(os.path.join(self.results_path, save_file), 'a') as f:
            f.write(datetime.datetime.now().strftime("%Y-%m-%d %H:%M:%S") + '\n')
            f.write(str(self.args_general) + '\n')
            for i in range(self.upsample + 1):
                f.write(f"Number of upsampling times: {i}\n")
                f.write(self._lines(i, J_totals, J_targets, J_energys, mses, n_l2s) + '\n')
            f.write("-----------------------------------------------------------------------------------------\n")

    def per_evaluate(self, sim, eval_no, pred, data, output_queue):
        """The reference's per-process worker (inference_2d.py:310-328). Nothing here starts it; called directly, it scores one sample in
        this process and puts {eval_no: solver outputs} on the queue."""
        from dataset.evaluate_solver import init_velocity_, solver
        if self.args_general.is_condition_control:
            _unsupported('per_evaluate with is_condition_control=True (the reference leaves its result undefined)', '315-325')
        p = np.asarray(pred)
        output_queue.put({eval_no: solver(sim, init_velocity_(), np.asarray(data)[0, 0], p[:, 3], p[:, 4])})

    def multi_evaluate_control(self, pred, data, plot=False):
        """solver_out [B, 256, 6, 128, 128] (float64 numpy, as the reference returns it) from one launch in this process."""
        from wdno_amd import smoke_solver
        if plot:
            _unsupported('plot=True', '372-378')
        print("Start solving...")
        return smoke_solver.evaluate_controls(pred.to(self.device), data.to(self.device)).cpu().numpy().astype(float)

    def multi_evaluate(self, pred, data, plot=False):
        """pred [B, nt, 6, nx, nx]; data: control [B, 256, 6, nx, nx], simulation [B, nt, 6, 128, 128]. Returns the reference's five arrays of
        one entry: J_total, J_target, J_energy, mse, n_l2 (batch means). As in the reference, pred[:, 0, 0] is overwritten with the data's.
        With is_super_model (simulation mode, inference_2d.py:405-456) pred is one level of the cascade and the five arrays have four entries:
        base, current, linear and nearest super resolution, with mse_wo_smoke in the mse slot (l.447-448)."""
        from wdno_amd.smoke import score as S
        if plot:
            _unsupported('plot=True', '372-378')
        sp = int(data.shape[-1] / pred.shape[-1])
        pred[:, 0, 0] = data[:, 0, 0, ::sp, ::sp].to(pred.device, pred.dtype)      # initial condition
        w = self.args_general.w_energy
        if getattr(self.args_general, 'is_super_model', False):
            if not self.args_general.is_condition_control:
                _unsupported('is_super_model=True with is_condition_control=False', '157')
            d = data.to(pred.device)
            if d.dtype not in (torch.float32, torch.float64):
                d = d.to(torch.float32)
            r = S.score_super(pred.to(torch.float32), d, w)
            T, n, N = pred.shape[1], pred.shape[3], d.shape[-1]
            print('current resolution:', T, n, n)
            for i, (msg, g) in enumerate(zip(('base resolution', 'current resolution', 'linear super resolution', 'nearest super resolution'),
                                             (N // 2, n, N, N))):
                print(msg, ', evaluate shape:', T, g, g)
                print('mse =', r['mse'][i].mean(), 'mse_wo_smoke =', r['mse_wo_smoke'][i].mean(), 'normalized_l2 =', r['n_l2'][i].mean())
            return tuple(r[k].mean(1) for k in ('J_total', 'J_target', 'J_energy', 'mse_wo_smoke', 'n_l2'))
        if not self.args_general.is_condition_control:
            start = time.time()
            r = S.score_controls(pred, data, w)
            print(f"Time cost: {time.time() - start}")
        else:
            d = data.to(pred.device)
            if d.dtype not in (torch.float32, torch.float64):
                d = d.to(torch.float32)
            r = S.score(pred.to(torch.float32), [d[:, :, c, ::sp, ::sp] for c in range(6)], w)
        print('current resolution', ', evaluate shape:', pred.shape[1], pred.shape[3], pred.shape[4])
        if not self.args_general.is_condition_control:
            print('J_total=J_target+w*J_energy=', r['J_target'].mean(), '+', w, '*', r['J_energy'].mean(), '=', r['J_total'].mean())
        print('mse =', r['mse'].mean(), 'mse_wo_smoke =', r['mse_wo_smoke'].mean(), 'normalized_l2 =', r['n_l2'].mean())
        return tuple(np.array([r[k].mean()]) for k in ('J_total', 'J_target', 'J_energy', 'mse', 'n_l2'))


def inference(dataloader, diffusion, design_fn, args, RESCALER):
    model_args = {"design_fn": design_fn, "design_guidance": args.design_guidance}
    InferencePipeline(diffusion, model_args, RESCALER, results_path=args.inference_result_subpath, args_general=args).run(dataloader)


def main(args):
    from ddpm.utils import load_data
    dataloader, shape, ori_shape, RESCALER = load_data(args)
    diffusion, design_fn = load_model(args, shape, ori_shape, RESCALER)
    inference(dataloader, diffusion, design_fn, args, RESCALER)


def build_parser():
    """The reference's argument parser (inference_2d.py:483-542): the same options, types and defaults."""
    p = argparse.ArgumentParser(description='inference 2d inverse design model')
    for name, kw in (
            ('--seed', dict(type=int, default=0, metavar='S')), ('--dataset', dict(default='Smoke', type=str)),
            ('--dataset_path', dict(default="./data/2d", type=str)), ('--w_energy', dict(default=0., type=float)),
            ('--image_size', dict(type=int, default=64)), ('--is_super_model', dict(default=False, type=eval)),
            ('--upsample', dict(default=0, type=int)), ('--inference_result_path', dict(default="./results/test/", type=str)),
            ('--batch_size', dict(default=50, type=int)), ('--exp_id', dict(default="base_sim", type=str)),
            ('--diffusion_model_path', dict(default="./results/train/", type=str)), ('--diffusion_checkpoint', dict(default=50, type=int)),
            ('--super_exp_id', dict(default="super_sim", type=str)), ('--super_diffusion_model_path', dict(default="./results/train/", type=str)),
            ('--super_diffusion_checkpoint', dict(default=75, type=int)), ('--is_condition_control', dict(default=False, type=eval)),
            ('--is_condition_pad', dict(default=True, type=eval)), ('--using_ddim', dict(default=False, type=eval)),
            ('--ddim_eta', dict(default=1., type=float)), ('--ddim_sampling_steps', dict(default=100, type=int)),
            ('--design_guidance', dict(default='standard', type=str)),
            ('--standard_fixed_ratio_list', dict(nargs='+', default=[0], type=float)), ('--coeff_ratio_list', dict(nargs='+', default=[0], type=float)),
            ('--w_init_list', dict(nargs='+', default=[0], type=float)), ('--is_wavelet', dict(default=False, type=eval)),
            ('--wave_type', dict(default='bior1.3', type=str)), ('--pad_mode', dict(default='zero', type=str))):
        p.add_argument(name, **kw)
    return p


def __getattr__(name):          # anything else of the reference module
    return _reference_getattr(name)


if __name__ == '__main__':
    args = build_parser().parse_args()
    torch.manual_seed(args.seed)
    torch.cuda.manual_seed(args.seed)
    np.random.seed(args.seed)
    args.device = torch.device('cuda') if torch.cuda.is_available() else torch.device('cpu')
    for w_init in args.w_init_list:
        for standard_fixed_ratio in args.standard_fixed_ratio_list:
            for coeff_ratio in args.coeff_ratio_list:
                current_time = datetime.datetime.now().strftime('%Y-%m-%d_%H-%M-%S')
                args.standard_fixed_ratio, args.coeff_ratio, args.w_init = standard_fixed_ratio, coeff_ratio, w_init
                args.inference_result_subpath = os.path.join(
                    args.inference_result_path,
                    current_time + f"_standard_fixed_ratio_{standard_fixed_ratio}_coeff_ratio_{coeff_ratio}_w_init_{w_init}_w_energy_{args.w_energy}",
                    args.inference_result_path)
                print("args: ", args)
                main(args)
