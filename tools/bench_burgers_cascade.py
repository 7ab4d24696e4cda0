"""Timings of the Burgers cascade's hand-off launch and of one whole cascade batch on one GPU (profiles/burgers_cascade.md):

  --handoff       wdno_amd.burgers.cascade.super_conditions (one launch) at batch 50, level 1 -- previous block [50, 8, 41, 60], source
                  [50, 17, 128, 128] -- against the chain it replaces, on the operators the tree had before: upsample_coef, the pad, the
                  division, get_target(is_wave=True, N_upsample=1) with the file held, its two slices and divisions, and the zeroed tensor
                  and three copies of GaussianDiffusion._sampling_setup. Device events around `--iters` back-to-back calls per window,
                  5 windows, the arms alternating inside each window, every arm run once untimed, one process;
                  spread = (max - min) / median. Kernel launches of one call of each arm are counted with torch.profiler.
  --batch-split   one whole evaluate() batch with upsample_x = 1 and full-size models (base dim 128, super_dim 64, (1, 2, 4, 8), random
                  weights, 1000 DDPM steps per level), split into sampling per level, solver per level and everything else;
                  the super level's sampling rate at [B, 17, 128, 128]; and the kernel routes one U-Net forward of that shape reached
                  (ops.PROFILE) with the plans of its attention layers.
Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wdno_amd import tree_path  # noqa: E402

for _t in ('third_party', 'burgers'):
    sys.path.insert(0, tree_path(_t))
from tools.bench_burgers_eval import _launches, _window  # noqa: E402
from wdno_amd.burgers import cascade as CS  # noqa: E402

SHAPE0, SHAPE1, PAD = (41, 60), (81, 120), 128


def _arms(what, arms, iters, **extra):
    for fn in arms.values():
        fn()
    t = {k: [] for k in arms}
    for _ in range(5):
        for k, fn in arms.items():
            t[k].append(_window(fn, iters))
    out = dict(what=what, iters=iters, **extra)
    for k, v in t.items():
        med = float(np.median(v))
        out[k] = dict(median_ms=med, spread_pct=100 * (max(v) - min(v)) / med, windows_ms=[round(w, 4) for w in v], launches=_launches(arms[k]))
    diff = out['chain']['median_ms'] - out['kernel']['median_ms']
    out['difference_ms'] = diff
    out['sum_of_spreads_ms'] = (out['chain']['spread_pct'] * out['chain']['median_ms'] + out['kernel']['spread_pct'] * out['kernel']['median_ms']) / 100
    out['meets_bar'] = bool(diff > out['sum_of_spreads_ms'])
    print(json.dumps(out), flush=True)


def bench_handoff(batch, iters):
    import eval_ddpm_burgers as E
    from ddpm_burgers import test_util as TU
    from ddpm_burgers.wavelet_utils import upsample_coef
    args = E.build_parser().parse_args(['--exp_id', 'bench', '--is_condition_u0', 'True', '--is_condition_uT', 'True', '--is_super_model', 'True',
                                        '--upsample_t', '1', '--upsample_x', '1'])
    resc = E.rescaler_table(args).cuda()
    idx = list(range(batch))
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            os.makedirs('data/1d_super')
            gen = torch.Generator().manual_seed(3)
            torch.save({'u': 0.3 * torch.randn(batch, 161, 240, generator=gen), 'f': 0.3 * torch.randn(batch, 160, 240, generator=gen)}, 'data/1d_super/test')
            g = torch.Generator(device='cuda').manual_seed(1)
            sample = torch.randn(batch, 9, 64, 64, device='cuda', generator=g) * 0.4
            x_prev = sample[:, :8, :SHAPE0[0], :SHAPE0[1]] * resc[:, 8:16]            # what diffuse_2dconv returns: the rescaled block, contiguous
            resc_f32 = resc.to(torch.float32).reshape(-1).contiguous()                  # as evaluate() casts the int64 table: once

            def chain():
                coef = upsample_coef(x_prev, SHAPE1)
                coef = F.pad(coef, (0, PAD - coef.shape[-1], 0, PAD - coef.shape[-2]), 'constant', 0)
                low = coef / resc[:, 8:16]
                u_condition = TU.get_target(args, is_wave=True, target_i=idx, N_upsample=1, dataset='1d')
                u_init, u_final = u_condition[:, :PAD // 2] / resc.squeeze()[-1], u_condition[:, -PAD // 2:] / resc.squeeze()[-1]
                src = torch.zeros((batch, 17, PAD, PAD), device='cuda', dtype=torch.float32)          # _sampling_setup
                ch, cw = SHAPE1[0] + 1, SHAPE1[1]
                src[:, -1, :PAD // 2, :cw] = u_init[:, :, :cw]
                src[:, -1, -PAD // 2:, :cw] = u_final[:, :, :cw]
                src[:, 8:16, :ch, :cw] = low[:, :, :ch, :cw]
                return src

            def kernel():
                return CS.super_conditions(x_prev, CS.get_target_view(args, idx, N_upsample=1, dataset='1d'), resc_f32, SHAPE1, PAD, PAD, True, True)
            a, b = kernel(), chain()
            low_equal = bool(torch.equal(a[:, :16], b[:, :16]))
            rel = float((a[:, 16] - b[:, 16]).abs().max() / b[:, 16].abs().max())
            _arms('handoff', {'kernel': kernel, 'chain': chain}, iters, batch=batch, source_mb=a.numel() * 4 / 1e6, low_bits_equal=low_equal,
                  condition_bits_equal=bool(torch.equal(a[:, 16], b[:, 16])), condition_relmax=rel)
        finally:
            os.chdir(cwd)


def bench_batch(batch):
    import eval_ddpm_burgers as E
    from ddpm_burgers import test_util as TU
    from wdno_amd import ops
    args = E.build_parser().parse_args(['--exp_id', 'bench', '--super_exp_id', 'bench_sr', '--is_condition_u0', 'True', '--is_condition_uT', 'True',
                                        '--is_super_model', 'True', '--upsample_t', '1', '--upsample_x', '1'])
    resc = E.rescaler_table(args)
    timers = {}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            os.makedirs('data/1d_super')
            gen = torch.Generator().manual_seed(3)
            torch.save({'u': 0.3 * torch.randn(batch, 161, 240, generator=gen), 'f': 0.3 * torch.randn(batch, 160, 240, generator=gen)}, 'data/1d_super/test')
            torch.manual_seed(0)
            ddpm = TU.get_2d_ddpm([41, 60], [81, 120], args, resc[:, 8:], is_super_model=False).cuda()
            args.dim = args.super_dim
            ddpm_super = TU.get_2d_ddpm(*CS.super_shapes([41, 60], [81, 120], 1), args, resc, is_super_model=True, upsample_t=1, upsample_x=1).cuda()
            E.load_2dconv_base_model = lambda model_i, a, r: ddpm
            E.load_2dconv_super_model = lambda model_i, a, r: ddpm_super
            real_solve = E.burgers_numeric_solve_free

            def timed(key, fn):
                def run(*a, **k):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = fn(*a, **k)
                    torch.cuda.synchronize()
                    name = key if key != 'solver' else f'solver_{int(np.log2(k["num_t"] // 80))}'
                    timers[name] = timers.get(name, 0.0) + time.perf_counter() - t0
                    return out
                return run
            ddpm.sample = timed('sampling_0', ddpm.sample)
            ddpm_super.sample_with_source = timed('sampling_1', ddpm_super.sample_with_source)
            E.burgers_numeric_solve_free = timed('solver', real_solve)
            out = dict(what='batch', batch=batch, steps=ddpm.num_timesteps, super_shape=[batch, 17, PAD, PAD])
            for run in ('first', 'second'):          # the first call captures the steps and reads the file; the second is the steady state
                timers.clear()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                E.evaluate('bench', 'bench_sr', args, Ntest=batch, batch_size=batch, wu=0.5, wf=0.01, RESCALER=resc)
                torch.cuda.synchronize()
                total = time.perf_counter() - t0
                out[run] = dict(total_s=total, **{k + '_s': v for k, v in sorted(timers.items())}, rest_s=total - sum(timers.values()))
            out['super_steps_per_s'] = ddpm_super.num_timesteps / out['second']['sampling_1_s']
            out['super_ms_per_step'] = 1e3 * out['second']['sampling_1_s'] / ddpm_super.num_timesteps
            out['base_ms_per_step'] = 1e3 * out['second']['sampling_0_s'] / ddpm.num_timesteps
            # the routes one forward of the super model's U-Net reaches at this shape
            x = torch.randn(batch, 17, PAD, PAD, device='cuda')
            t = torch.full((batch,), 500, device='cuda', dtype=torch.long)
            with torch.no_grad():
                ddpm_super.model(x, t, None)
                ops.PROFILE = {}
                ddpm_super.model(x, t, None)
                torch.cuda.synchronize()
                out['unet_routes'] = {k: len(v) for k, v in sorted(ops.PROFILE.items())}
                ops.PROFILE = None
            out['mid_attention_plan'] = ops.attn_plan('fwd', 4, batch, 1, (PAD // 8) ** 2)
            out['linear_attention_plans'] = {str(PAD // 2 ** i): ops.linattn_plan(batch, (PAD // 2 ** i) ** 2, 4) for i in range(4)}
            print(json.dumps(out, default=str), flush=True)
        finally:
            os.chdir(cwd)
            E.burgers_numeric_solve_free = real_solve


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--handoff', action='store_true')
    ap.add_argument('--batch-split', action='store_true')
    ap.add_argument('--batch', type=int, default=50)
    ap.add_argument('--iters', type=int, default=50)
    a = ap.parse_args()
    if a.handoff:
        bench_handoff(a.batch, a.iters)
    if a.batch_split:
        bench_batch(a.batch)
