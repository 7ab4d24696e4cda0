"""Time the smoke control-evaluation solver (wdno_amd.smoke_solver.solve, one launch of csrc/smoke_solver.hip: 256 frames x up to 500 CG
iterations per simulation) at batch 1, the evaluation batch (inference_2d.py --batch_size, 50) and 256, against a torch restatement of the
reference's frame loop on the same GPU.

Device events around each call after one warm-up call; the median of --reps calls. Only the last frame is written (frames=[255]), as the
full density and velocity are 50 MB per simulation; --full-outputs times batch 1 and the evaluation batch with every frame written.
The torch form is the frame loop in fp32 with slices and a 500-iteration CG of torch ops (no early exit: the reference runs 499.9 of 500
on average); its first --torch-frames frames are timed and scaled by 256 / frames (EXTRAPOLATED).
--sweep times every supported workgroup size at every batch (median of 3). One JSON line per measurement.

    python tools/bench_smoke_solver.py [--reps 5] [--sweep] [--torch] [--full-outputs]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wdno_amd import smoke_solver as W  # noqa: E402

BATCHES = (1, 50, 256)
NT, NX = 32, 64


def inputs(B):
    """The fixtures' kind of input: a density blob above the target bucket, rim-only controls (normal on 8 x 8, x 0.3, repeated 8 x)."""
    g = torch.Generator(device='cuda').manual_seed(1)
    d0 = torch.zeros(B, NX, NX, device='cuda')
    d0[:, 40:48, 28:36] = 1
    c = torch.randn(2, B, NT, 8, 8, device='cuda', generator=g) * 0.3
    c = c.repeat_interleave(8, -1).repeat_interleave(8, -2)
    c[..., 8:56, 8:56] = 0
    return d0, c[0].contiguous(), c[1].contiguous()


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


def torch_form_ms(d0, c1, c2, frames):
    """The reference's frame loop for the batch in fp32 torch ops (velocity composition, mask, divergence, 500 CG iterations with the masked
    5-point stencil as slices, projection, bilinear advection of both densities by gather), `frames` frames; returns ms."""
    geom = W.geometry()
    B = d0.shape[0]
    st = {k: torch.from_numpy(v).cuda() for k, v in geom.stencil().items()}
    vmask = torch.from_numpy(geom.velocity_mask.astype(np.float32)).cuda()
    C1, C2 = W.tile_control(c1, range(frames)), W.tile_control(c2, range(frames))
    v0 = torch.from_numpy(W.init_velocity()).cuda().expand(B, -1, -1, -1).contiguous()
    dens0 = d0.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :-1, :-1].contiguous()
    ii, jj = torch.meshgrid(torch.arange(127., device='cuda'), torch.arange(127., device='cuda'), indexing='ij')

    def apply_A(p):
        out = st['centre'] * p
        out[:, 1:, :] += st['up'][1:, :] * p[:, :-1, :]
        out[:, :, 1:] += st['left'][:, 1:] * p[:, :, :-1]
        out[:, :, :-1] += st['right'][:, :-1] * p[:, :, 1:]
        out[:, :-1, :] += st['down'][:-1, :] * p[:, 1:, :]
        return out

    def advect(f, v):
        ci = (v[:, 1:, :-1, 1] + v[:, :-1, :-1, 1]) / 2
        cj = (v[:, :-1, 1:, 0] + v[:, :-1, :-1, 0]) / 2
        yi, xj = (ii - ci).clamp(0, 127), (jj - cj).clamp(0, 127)
        inside = (yi <= 126) & (xj <= 126)
        i0, j0 = yi.floor().clamp(max=125).long(), xj.floor().clamp(max=125).long()
        wy, wx = yi - i0, xj - j0
        flat = f.reshape(B, -1)
        at = lambda a, b: flat.gather(1, (a * 127 + b).reshape(B, -1)).reshape(B, 127, 127)
        val = (1 - wy) * (1 - wx) * at(i0, j0) + (1 - wy) * wx * at(i0, j0 + 1) + wy * (1 - wx) * at(i0 + 1, j0) + wy * wx * at(i0 + 1, j0 + 1)
        return torch.where(inside, val, torch.zeros_like(val))

    def run():
        vel, dens, zdens = v0, dens0, dens0
        for frame in range(frames):
            cur = torch.stack([C1[:, frame], C2[:, frame]], -1)
            cur[:, 16:112, 16:112] = vel[:, 16:112, 16:112]
            cur = cur * vmask
            r = (cur[:, 1:, :-1, 1] - cur[:, :-1, :-1, 1]) + (cur[:, :-1, 1:, 0] - cur[:, :-1, :-1, 0])
            x, p = torch.zeros_like(r), r
            Ap = apply_A(p)
            for _ in range(500):
                tmp = (p * Ap).sum((1, 2), keepdim=True)
                a = (p * r).sum((1, 2), keepdim=True) / tmp
                x = x + a * p
                r = r - a * Ap
                b = -(r * Ap).sum((1, 2), keepdim=True) / tmp
                p = r + b * p
                Ap = apply_A(p)
            pp = F.pad(x[:, None], (1, 1, 1, 1), mode='replicate')[:, 0]
            grad = torch.stack([pp[:, 1:, 1:] - pp[:, 1:, :-1], pp[:, 1:, 1:] - pp[:, :-1, 1:]], -1)
            vel = (cur - grad * vmask) * vmask
            dens, zdens = advect(dens, vel), advect(zdens, vel)
        return dens
    ms, _ = time_calls(run, 1)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sweep', action='store_true')
    ap.add_argument('--torch', action='store_true')
    ap.add_argument('--torch-frames', type=int, default=2)
    ap.add_argument('--full-outputs', action='store_true')
    a = ap.parse_args()
    iters = W.NUM_T * W.MAX_ITER
    for B in BATCHES:
        d0, c1, c2 = inputs(B)
        med, ms = time_calls(lambda: W.solve(d0, c1, c2, frames=[255]), a.reps)
        rec = dict(batch=B, threads=W.DEFAULT_THREADS, median_ms=round(med, 2), calls_ms=[round(x, 2) for x in ms],
                   us_per_cg_iteration=round(med * 1e3 / iters, 3), cycles_per_cg_iteration_at_2400MHz=round(med * 1e-3 * 2.4e9 / iters))
        if a.torch:
            tms = torch_form_ms(d0, c1, c2, a.torch_frames)
            rec['torch_form_ms_extrapolated'] = round(tms * W.NUM_T / a.torch_frames, 1)
            rec[f'torch_form_ms_{a.torch_frames}_frames'] = round(tms, 2)
            rec['speedup_vs_torch_form_extrapolated'] = round(tms * W.NUM_T / a.torch_frames / med, 1)
        print(json.dumps(rec), flush=True)
        if a.full_outputs and B <= 50:
            m, _ = time_calls(lambda: W.solve(d0, c1, c2), 3)
            print(json.dumps(dict(batch=B, full_outputs=True, median_ms=round(m, 2))), flush=True)
        if a.sweep:
            for threads in W.THREADS:
                m, _ = time_calls(lambda: W.solve(d0, c1, c2, frames=[255], threads=threads), 3)
                print(json.dumps(dict(batch=B, sweep_threads=threads, median_ms=round(m, 2),
                                      cycles_per_cg_iteration_at_2400MHz=round(m * 1e-3 * 2.4e9 / iters))), flush=True)
        del d0, c1, c2
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
