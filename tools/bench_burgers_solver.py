"""Time the Burgers control-evaluation solver (wdno_amd.burgers_solver.solve, one launch of csrc/burgers.hip) at the two shapes of the
reference's workflow, against a torch restatement of the reference loop on the same GPU.

  evaluation     : N = 25, u0 [25, 120], f [25, 80, 120] -> [25, 81, 1920], T = 8 (eval_ddpm_burgers.py:203 of the base model)
  data generation: N = 800, u0 [800, 1920], f [800, 1280, 1920] (7.9 GB, drawn on the device from a seed), num_t = 320, T = 8
                   (generate_burgers.py's batch of 800)

Device events around each call after one warm-up call; the median of --reps calls. The torch form is the reference's fp32 loop restated with
slices (the same operations per step, ~12 launches): its first 7 680 steps are timed and scaled by 614 400 / 7 680 = 80 (EXTRAPOLATED).
--sweep times every supported (W, P) at both shapes (median of 3). One JSON line per measurement.

    python tools/bench_burgers_solver.py [--reps 5] [--sweep] [--torch] [--only eval|datagen]
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wdno_amd import burgers_solver as B  # noqa: E402

T, VISC = 8.0, 0.01


def inputs(shape):
    g = torch.Generator(device='cuda').manual_seed(0)
    if shape == 'eval':
        N, nx, Nt_f, num_t, ds = 25, 120, 80, 80, False
    else:
        N, nx, Nt_f, num_t, ds = 800, 1920, 1280, 320, True
    x = torch.linspace(0, 1, nx, device='cuda')
    u0 = (torch.rand(N, 1, device='cuda', generator=g) * 2) * torch.exp(-0.5 * (x - 0.3) ** 2 / 0.01)
    f = torch.empty(N, Nt_f, nx, device='cuda')
    for i in range(0, N, 100):            # in slices: no [N, Nt_f, nx] temporaries beside the 7.9 GB tensor
        n = min(100, N - i)
        amp = torch.rand(n, 1, 1, device='cuda', generator=g) * 3 - 1.5
        loc = torch.rand(n, 1, 1, device='cuda', generator=g)
        ts = torch.linspace(0, 1, Nt_f, device='cuda').view(1, -1, 1)
        f[i:i + n] = amp * torch.exp(-0.5 * (x - loc) ** 2 / 0.04) * torch.exp(-0.5 * (ts - loc) ** 2 / 0.09)
    return u0, f, dict(visc=VISC, T=T, num_t=num_t, output_space_downsample=ds)


def time_calls(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), ms


def torch_form_ms(u0, f, kw, steps_timed=7680):
    """The reference loop (generate_burgers.py:176-195) in fp32 with slices, its first `steps_timed` steps; returns (ms, steps of a call)."""
    s = 1920
    u = F.interpolate(u0[:, None], size=s, mode='linear', align_corners=False)[:, 0]
    fi = F.interpolate(f[:, :1], size=s, mode='linear', align_corners=False)      # the first interval's slice: all the timed steps use it
    dx = 1.0 / (s + 1)
    c, d, dm = (float(np.float32(v)) for v in (1.0 / (2 * dx), VISC / dx ** 2, VISC * -2.0 / dx ** 2))
    dt = float(np.float32(1 / 76800))
    steps = math.ceil(T / (1 / 76800))
    record_time = steps // kw['num_t']
    sol = torch.zeros(u.shape[0], s, kw['num_t'], device='cuda')

    def run():
        uu = u
        for j in range(steps_timed):
            up = F.pad(uu, (1, 1))
            a, e = up[:, :-2], up[:, 2:]
            uu = uu + dt * (-0.5 * ((a * a) * (-c) + (e * e) * c) + (a * d + uu * dm + e * d) + fi[:, 0])
            if (j + 1) % record_time == 0:
                sol[..., (j + 1) // record_time - 1] = uu
        return uu
    ms, _ = time_calls(run, 3)
    return ms, steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sweep', action='store_true')
    ap.add_argument('--torch', action='store_true')
    ap.add_argument('--only', choices=['eval', 'datagen'])
    a = ap.parse_args()
    props = torch.cuda.get_device_properties(0)
    cus = props.multi_processor_count
    for shape in ('eval', 'datagen'):
        if a.only and shape != a.only:
            continue
        u0, f, kw = inputs(shape)
        pl = B.plan(tuple(u0.shape), tuple(f.shape), kw['T'], num_t=kw['num_t'], output_space_downsample=kw['output_space_downsample'],
                    cu_count=cus)
        med, ms = time_calls(lambda: B.solve(u0, f, **kw), a.reps)
        rec = dict(shape=shape, N=pl['N'], f=list(f.shape), steps=pl['steps'], config=[pl['waves'], pl['points']], median_ms=round(med, 3),
                   calls_ms=[round(x, 3) for x in ms])
        if a.torch:
            tms, steps = torch_form_ms(u0, f, kw)
            rec['torch_form_ms_extrapolated'] = round(tms * steps / 7680, 1)
            rec['torch_form_ms_7680_steps'] = round(tms, 2)
            rec['speedup_vs_torch_form_extrapolated'] = round(tms * steps / 7680 / med, 1)
        print(json.dumps(rec), flush=True)
        if a.sweep:
            for cfg in B.configs(pl['s']):
                m, _ = time_calls(lambda: B.solve(u0, f, config=cfg, **kw), 3)
                print(json.dumps(dict(shape=shape, sweep=list(cfg), median_ms=round(m, 3),
                                      cycles_per_step_at_2400MHz=round(m * 1e-3 * 2.4e9 / pl['steps']))), flush=True)
        del u0, f
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
