"""Time guided Burgers sampling at the evaluation's shape -- batch 50 (eval_ddpm_burgers.py:38-41), x [50, 9, 64, 64], the full-size
Unet2D(dim=128, dim_mults=(1, 2, 4, 8)) with random weights, coefficient block 41 x 60, fields 81 x 120 -- in three arms that alternate inside
one process:

  new       sample(nablaJ=BurgersGuidance(...)): U-Net -> one guidance launch -> fused update, every noisy step a replay of one HIP graph
  old       the previous route: nablaJ = get_nablaJ(guidance_value) (autograd through the DWT adjoint kernels) on the eager loop
  unguided  the replayed unguided loop, same shape

A step is timed as an ancestral chain of --steps timesteps divided by its length (the public sample() call: conditions, final eager step and
the noise draws included in every arm alike); --ddim adds the DDIM-100 chain of 1000 timesteps end to end. Inputs are drawn on the device
from a seed; every arm runs once before it is timed (graph capture, operand caches); device events; --windows >= 5 windows per arm, median
and spread (max - min over the median) reported. One JSON line per measurement.

  --kernel N   instead: N launches of the guidance kernel (fused mode) and N calls of the old route's nablaJ, nothing else -- the run to put
               under `rocprofv3 --kernel-trace --stats -- python tools/bench_burgers_guidance.py --kernel 20` (the names to look for are
               burgers_guidance_kernel and, for the old route, everything else in the trace).

    python tools/bench_burgers_guidance.py [--steps 20] [--windows 5] [--ddim] [--batch 50] [--kernel N]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wdno_amd import tree_path  # noqa: E402

for _t in ('third_party', 'burgers'):
    sys.path.insert(0, tree_path(_t))
from ddpm_burgers import model_utils as MU  # noqa: E402
from ddpm_burgers.diffusion_1d import GaussianDiffusion  # noqa: E402
from ddpm_burgers.unet import Unet2D  # noqa: E402
from wdno_amd.burgers import guidance as BG  # noqa: E402

DEV = 'cuda'
SHAPE, ORI = (41, 60), (81, 120)
RESCALER = [10, 3, 3, 1, 21, 5, 5, 1, 10]
WU, WF = 0.7, 0.03


def build(net, timesteps, sampling_timesteps=None):
    return GaussianDiffusion(net, seq_length=(64, 64), pad_mode='periodization', wave_type='bior2.4', padded_shape=list(SHAPE), ori_shape=list(ORI),
                             timesteps=timesteps, sampling_timesteps=sampling_timesteps, ddim_sampling_eta=0., is_condition_pad=True,
                             is_condition_u0=True).to(DEV)


def inputs(batch):
    g = torch.Generator(device=DEV).manual_seed(0)
    u_target = torch.randn(batch, ORI[0], ORI[1], device=DEV, generator=g)
    u_init = torch.randn(batch, 32, 64, device=DEV, generator=g) * 0.3
    resc = torch.tensor(RESCALER, dtype=torch.float32, device=DEV).reshape(1, 9, 1, 1)
    return u_target, u_init, resc


def arms(batch, u_target, u_init, resc):
    new = BG.BurgersGuidance(SHAPE, ORI, resc, u_target, WU, WF)
    old = MU.get_nablaJ(lambda x: BG.guidance_value(x, u_target, SHAPE, ORI, resc, WU, WF))
    sched = lambda t: 0.1
    return {'new': dict(batch_size=batch, u_init=u_init, nablaJ=new, J_scheduler=sched),
            'old': dict(batch_size=batch, u_init=u_init, nablaJ=old, J_scheduler=sched),
            'unguided': dict(batch_size=batch, u_init=u_init)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(dif, kws, windows, tag, per):
    for kw in kws.values():                  # warm-up of every timed arm: graph capture, packed weights, descriptors
        dif.sample(**kw)
    torch.cuda.synchronize()
    ms = {k: [] for k in kws}
    for _ in range(windows):
        for k, kw in kws.items():            # the arms alternate inside a window
            ms[k].append(timed(lambda: dif.sample(**kw)) / per)
    out = {}
    for k, v in ms.items():
        med = statistics.median(v)
        out[k] = med
        print(json.dumps(dict(measurement=tag, arm=k, unit='ms per step' if per > 1 else 'ms', median=round(med, 4),
                              spread=round((max(v) - min(v)) / med, 4), windows=[round(x, 4) for x in v])), flush=True)
    return out


def kernel_only(n, batch):
    u_target, u_init, resc = inputs(batch)
    kws = arms(batch, u_target, u_init, resc)
    from wdno_amd import diffusion_core as K

    class Sched(torch.nn.Module):
        def __init__(self):
            super().__init__()
            K.register_schedule(self, K.cosine_beta_schedule(1000), lambda snr: torch.ones_like(snr))
    mod = Sched().to(DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    x_t = torch.randn(batch, 9, 64, 64, device=DEV, generator=g)
    eps = torch.randn(batch, 9, 64, 64, device=DEV, generator=g)
    t = torch.full((batch,), 500, device=DEV, dtype=torch.long)
    s_table = torch.full((1000,), 0.1, device=DEV)
    new, old = kws['new']['nablaJ'], kws['old']['nablaJ']
    for _ in range(n):
        new.guide(mod, x_t, eps, t, s_table, False)
    torch.cuda.synchronize()
    ex = lambda a: a[t].reshape(batch, 1, 1, 1)
    for _ in range(n):                       # the old route's step: predict x0, nablaJ by autograd, scale, add (diffusion_1d.py: model_predictions)
        x0 = ex(mod.sqrt_recip_alphas_cumprod) * x_t - ex(mod.sqrt_recipm1_alphas_cumprod) * eps
        with torch.enable_grad():
            out = eps + old(x0) * 0.1
    torch.cuda.synchronize()
    print(json.dumps(dict(measurement='kernel-only', launches=n, batch=batch, bytes_per_launch=3 * x_t.numel() * 4)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--batch', type=int, default=50)
    ap.add_argument('--ddim', action='store_true')
    ap.add_argument('--kernel', type=int, default=0)
    a = ap.parse_args()
    if a.kernel:
        return kernel_only(a.kernel, a.batch)
    torch.manual_seed(0)
    net = Unet2D(dim=128, dim_mults=(1, 2, 4, 8), channels=9)
    u_target, u_init, resc = inputs(a.batch)
    kws = arms(a.batch, u_target, u_init, resc)
    dif = build(net, a.steps)
    dif.use_graph = True
    step = measure(dif, kws, max(a.windows, 5), f'ancestral step (chain of {a.steps} / {a.steps})', a.steps)
    print(json.dumps(dict(measurement='ratios', new_over_unguided=round(step['new'] / step['unguided'], 4),
                          old_over_new=round(step['old'] / step['new'], 3))), flush=True)
    if a.ddim:
        dif = build(net, 1000, 100)
        measure(dif, {k: kws[k] for k in ('new', 'old')}, max(a.windows, 5), 'DDIM-100 chain end to end', 1)


if __name__ == '__main__':
    main()
