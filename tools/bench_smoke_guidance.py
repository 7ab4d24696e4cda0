"""Time guided smoke sampling at the inference shape -- state [B, 24, 42, 40, 40], coefficient block (18, 34, 34), fields (32, 64, 64), the
full-size Unet3D_with_Conv3D(dim=64, dim_mults=(1, 2, 4)) with random weights, w_energy, w_init > 0 -- in three arms that alternate inside
one process:

  new       sample(design_fn=SmokeGuidance(...)): U-Net -> two guidance launches -> fused update, every noisy step a replay of one HIP graph
  old       sample(design_fn=GuidanceFn(...)): the previous graph route (torch element-wise glue around the IDWT / adjoint-IDWT launches)
  unguided  the replayed unguided loop, same shape

A step is timed as an ancestral chain of --steps timesteps divided by its length (the public sample() call: conditions, final eager step and
the noise draws included in every arm alike); --ddim adds a DDIM chain of --ddim sampling steps over 1000 timesteps, end to end. Inputs are
drawn on the device from a seed; every arm runs once before it is timed (graph capture, operand caches); device events; --windows >= 5
windows per arm (--repeat sample() calls per window: a window of a fraction of a second measures the clock as much as the step), median
and spread (max - min over the median) reported. One JSON line per measurement.

  --kernel N   instead: N calls of the new guidance (fused mode) and N of the old route's step glue (predict x0, GuidanceFn, scale, add),
               nothing else -- the run to put under `rocprofv3 --kernel-trace --stats -- python tools/bench_smoke_guidance.py --kernel 20`
               (the names to look for are smoke_guidance_synthesis_kernel / smoke_guidance_adjoint_kernel; everything else in the trace is
               the old route).

    python tools/bench_smoke_guidance.py [--steps 20] [--windows 5] [--repeat 1] [--ddim N] [--batch 8] [--kernel N]
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

for _t in ('third_party', 'smoke'):
    sys.path.insert(0, tree_path(_t))
from ddpm.diffusion_2d import GaussianDiffusion  # noqa: E402
from video_diffusion_pytorch.video_diffusion_pytorch_conv3d import Unet3D_with_Conv3D  # noqa: E402
from wdno_amd.smoke import guidance as Gd  # noqa: E402

DEV = 'cuda'
SHAPE, ORI = (18, 34, 34), (32, 64, 64)
W_E, W_I = 0.7, 1.3


def build(net, resc, timesteps, sampling_timesteps=None):
    dif = GaussianDiffusion(net, resc, False, True, True, False, 'bior1.3', 'zero', SHAPE, ORI, image_size=40, frames=24, timesteps=timesteps,
                            sampling_timesteps=sampling_timesteps, loss_type='l2', ddim_sampling_eta=1.0, standard_fixed_ratio=0.05).to(DEV)
    dif.use_graph = True
    return dif


def inputs(batch):
    g = torch.Generator(device=DEV).manual_seed(0)
    init = torch.randn(batch, 24, 40, 40, device=DEV, generator=g) * 0.3
    init_u = torch.randn(batch, ORI[1], ORI[2], device=DEV, generator=g)
    resc = torch.linspace(1.0, 22.0, 42, device=DEV).reshape(1, 1, 42, 1, 1)
    return init, init_u, resc


def arms(batch, init, init_u, resc):
    kw = dict(w_energy=W_E, w_init=W_I)
    base = dict(batch_size=batch, init=init)
    return {'new': dict(base, init_u=init_u, design_fn=Gd.SmokeGuidance(SHAPE, ORI, resc, **kw), design_guidance='standard'),
            'old': dict(base, init_u=init_u, design_fn=Gd.GuidanceFn(SHAPE, ORI, resc, **kw), design_guidance='standard'),
            'unguided': base}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(dif, kws, windows, tag, per, repeat=1):
    for kw in kws.values():                  # warm-up of every timed arm: graph capture, packed weights, descriptors
        dif.sample(**kw)
    torch.cuda.synchronize()
    ms = {k: [] for k in kws}
    for _ in range(windows):
        for k, kw in kws.items():            # the arms alternate inside a window
            ms[k].append(timed(lambda: [dif.sample(**kw) for _ in range(repeat)]) / (per * repeat))
    out = {}
    for k, v in ms.items():
        med = statistics.median(v)
        out[k] = (med, (max(v) - min(v)) / med)
        print(json.dumps(dict(measurement=tag, arm=k, unit='ms per step' if per > 1 else 'ms', median=round(med, 4),
                              spread=round(out[k][1], 4), windows=[round(x, 4) for x in v])), flush=True)
    new, old, plain = out['new'], out['old'], out['unguided']
    print(json.dumps(dict(measurement=tag + ': ratios', new_over_unguided=round(new[0] / plain[0], 4), old_over_new=round(old[0] / new[0], 4),
                          old_minus_new_over_old=round((old[0] - new[0]) / old[0], 4), sum_of_spreads=round(new[1] + old[1], 4),
                          faster_by_more_than_the_spreads=bool((old[0] - new[0]) / old[0] > new[1] + old[1]))), flush=True)
    return out


def kernel_only(n, batch):
    from wdno_amd import diffusion_core as K
    init, init_u, resc = inputs(batch)
    kws = arms(batch, init, init_u, resc)

    class Sched(torch.nn.Module):
        def __init__(self):
            super().__init__()
            K.register_schedule(self, K.sigmoid_beta_schedule(1000), lambda snr: torch.ones_like(snr))
    mod = Sched().to(DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    x_t = torch.randn(batch, 24, 42, 40, 40, device=DEV, generator=g)
    eps = torch.randn(batch, 24, 42, 40, 40, device=DEV, generator=g)
    t = torch.full((batch,), 500, device=DEV, dtype=torch.long)
    s_table = torch.full((1000,), 0.05, device=DEV)
    new, old = kws['new']['design_fn'].set_init_u(init_u), kws['old']['design_fn']
    ex = lambda a: a[t].reshape(batch, 1, 1, 1, 1)
    ms = {}
    for name in ('new', 'old'):
        for timed_pass in (False, True):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                if name == 'new':
                    new.guide(mod, x_t, eps, t, s_table, True)
                else:                            # the old route's glue up to the guided noise (diffusion_2d.py: model_predictions)
                    x0 = (ex(mod.sqrt_recip_alphas_cumprod) * x_t - ex(mod.sqrt_recipm1_alphas_cumprod) * eps).clamp(-1., 1.)
                    eps + 0.05 * old(x0, init_u=init_u)
            e1.record()
            torch.cuda.synchronize()
            if timed_pass:
                ms[name] = e0.elapsed_time(e1) / n
    # a plain device copy of the state as the yardstick of the memory system: read + write of x_t
    torch.cuda.synchronize()
    dst = torch.empty_like(x_t)
    dst.copy_(x_t)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        dst.copy_(x_t)
    e1.record()
    torch.cuda.synchronize()
    copy_ms = e0.elapsed_time(e1) / n
    nbytes = x_t.numel() * 4
    print(json.dumps(dict(measurement='guidance only (host-issued, back to back)', calls=n, batch=batch, new_ms=round(ms['new'], 4),
                          old_ms=round(ms['old'], 4), state_copy_ms=round(copy_ms, 4), copy_GBps=round(2 * nbytes / copy_ms / 1e6, 1),
                          new_min_bytes=3 * nbytes, new_GBps_on_min_bytes=round(3 * nbytes / ms['new'] / 1e6, 1))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--ddim', type=int, default=0)
    ap.add_argument('--repeat', type=int, default=1)
    ap.add_argument('--kernel', type=int, default=0)
    a = ap.parse_args()
    if a.kernel:
        return kernel_only(a.kernel, a.batch)
    torch.manual_seed(0)
    net = Unet3D_with_Conv3D(dim=64, dim_mults=(1, 2, 4), channels=42)
    init, init_u, resc = inputs(a.batch)
    kws = arms(a.batch, init, init_u, resc)
    measure(build(net, resc, a.steps), kws, max(a.windows, 5), f'batch {a.batch}: ancestral step (chain of {a.steps} / {a.steps}, {a.repeat} per window)', a.steps,
            a.repeat)
    if a.ddim:
        measure(build(net, resc, 1000, a.ddim), kws, max(a.windows, 5), f'batch {a.batch}: DDIM-{a.ddim} chain end to end ({a.repeat} per window)', 1,
                a.repeat)


if __name__ == '__main__':
    main()
