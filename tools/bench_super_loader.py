"""Timings of the resident input pipeline of the super-resolution smoke models on one GPU (profiles/smoke_super_loader.md), at the reference's
level-0 size: fine [5, 8, 18, 34, 34] with coarse [5, 8, 10, 34, 34] (time) or [5, 8, 18, 18, 18] (space) -> state [B, 24, 82, 40, 40].

  (a) kernel      wdno_pack_smoke_super_state for a batch drawn by an index list from `--sims` resident simulations against the only device route
                  without it: pack_smoke_state(..., coef_sub=...) per sample on device tensors plus torch.stack. Per Python call (host enqueue
                  included) and per replay of 20 calls captured in one graph (the launches alone).
  (b) rate        bytes read plus written per microsecond of the kernel (graph figure of (a)), next to pack_smoke_state_kernel<0> on the base
                  shape [B, 24, 42, 40, 40] in the same run. A yardstick, not a gate.
  (c) step        the 82-channel training step (Unet3D_with_Conv3D(dim=64, (1, 2, 4)), graph replay) fed by ResidentSuperSmokeLoader in its
                  second epoch, by one resident state tensor, and by SuperDataLoader with the Trainer's default of 4 workers; synthetic files
                  in the offline transform's format on local disk. Gate: loader rate / tensor rate >= step / (step + kernel) - 0.01, all
                  three terms from this run (the pack shares the step's stream: its own time is the expected loss; 0.01 for host jitter).
Prints one JSON line per measurement; exit status 1 when a gate fails. `--kind`, `--batch` and `--skip-step` split the work into short runs."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wdno_amd import tree_path  # noqa: E402

for _t in ('third_party', 'smoke'):
    sys.path.insert(0, tree_path(_t))
from ddpm.data_2d import (Smoke_wave, SuperDataLoader, pack_smoke_gpu, pack_smoke_state, pack_smoke_super_gpu, _RESCALERS)  # noqa: E402
from wdno_amd.loader import ResidentSuperSmokeLoader  # noqa: E402

DEV = 'cuda'
FINE = (18, 34, 34)
COARSE = {'time': (10, 34, 34), 'space': (18, 18, 18)}


def _ev_time(fn, iters, warm=3):
    """Average duration in ms of fn() measured with device events on the launch stream."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def _both(fn):
    """ms per Python call (host enqueue included) and per call replayed from 20 calls captured in one graph (median of 5 windows of 10 replays)."""
    ms_call = _ev_time(fn, 20)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(20):
            fn()
    w = sorted(_ev_time(g.replay, 10) / 20 for _ in range(5))
    return ms_call, w[2], 100 * (w[-1] - w[0]) / w[2]


def write_files(root, kind, n):
    d = os.path.join(root, 'train', 'bior1.3_zero', f'{kind}_downsample')
    os.makedirs(d)
    g = torch.Generator().manual_seed(0)
    shapes = [FINE, COARSE[kind]]
    for i in range(n):
        torch.save({'coef': [torch.randn(5, 8, *s, generator=g) * 3 for s in shapes], 'init_coef': [torch.randn(5, 4, s[1], s[2], generator=g) for s in shapes],
                    'smokeout': [torch.rand(2, s[0], generator=g) for s in shapes], 'shape': shapes, 'ori_shape': (32, 64, 64)}, os.path.join(d, f'{i:06d}'))


def bench_kernel(kind, batch, sims):
    """(a) and (b). Returns the kernel's ms per batch (graph figure) for the gate of (c)."""
    g = torch.Generator(device=DEV).manual_seed(1)
    fine = torch.randn(sims, 5, 8, *FINE, device=DEV, generator=g) * 3
    coarse = torch.randn(sims, 5, 8, *COARSE[kind], device=DEV, generator=g) * 3
    init5 = torch.randn(sims, 5, 4, 34, 34, device=DEV, generator=g)
    so = torch.rand(sims, 2, 18, device=DEV, generator=g)
    r42 = torch.tensor(_RESCALERS['bior1.3'], dtype=torch.float32, device=DEV)
    r82 = torch.cat((r42[:40], r42[:40], r42[-2:]))
    pick = torch.randperm(sims, generator=torch.Generator().manual_seed(2))[:batch]
    idx, ids = pick.to(DEV), pick.tolist()
    kernel = lambda: pack_smoke_super_gpu(fine, coarse, init5, so, r82, kind, idx)
    chain = lambda: torch.stack([pack_smoke_state(fine[i], init5[i], so[i], r82.reshape(1, 82, 1, 1), coef_sub=coarse[i], downsample_type=kind) for i in ids])
    base = lambda: pack_smoke_gpu(fine, init5, so, r42, idx)
    assert torch.equal(kernel(), chain())
    k_call, k_graph, k_spread = _both(kernel)
    c_call, c_graph, c_spread = _both(chain)
    b_call, b_graph, b_spread = _both(base)
    per_sim = lambda *ts: sum(t[0].numel() for t in ts)
    k_bytes = 4 * batch * (per_sim(fine, coarse, so) + 4 * 34 * 34 + 24 * 82 * 40 * 40)
    b_bytes = 4 * batch * (per_sim(fine, so) + 4 * 34 * 34 + 24 * 42 * 40 * 40)
    k_rate, b_rate = k_bytes / (k_graph * 1e3), b_bytes / (b_graph * 1e3)
    print(json.dumps(dict(what='pack_super_kernel', kind=kind, batch=batch, resident_sims=sims,
                          kernel_ms_per_call=round(k_call, 4), kernel_ms_in_graph=round(k_graph, 5), kernel_graph_spread_pct=round(k_spread, 1),
                          per_sample_chain_ms_per_call=round(c_call, 4), per_sample_chain_ms_in_graph=round(c_graph, 5), chain_graph_spread_pct=round(c_spread, 1),
                          chain_over_kernel_in_graph=round(c_graph / k_graph, 2), chain_over_kernel_per_call=round(c_call / k_call, 2))), flush=True)
    print(json.dumps(dict(what='pack_super_rate', kind=kind, batch=batch, super_bytes=k_bytes, super_bytes_per_us=round(k_rate, 1),
                          base_kernel_ms_in_graph=round(b_graph, 5), base_graph_spread_pct=round(b_spread, 1), base_bytes=b_bytes,
                          base_bytes_per_us=round(b_rate, 1), super_over_base_rate=round(k_rate / b_rate, 3))), flush=True)
    return k_graph


def build_step(kind, batch):
    from ddpm.diffusion_2d import GaussianDiffusion
    from video_diffusion_pytorch.video_diffusion_pytorch_conv3d import Unet3D_with_Conv3D
    from wdno_amd.trainer import TrainStep, multistep_lr
    torch.manual_seed(0)
    net = Unet3D_with_Conv3D(dim=64, dim_mults=(1, 2, 4), channels=82)
    dif = GaussianDiffusion(net, torch.linspace(1.0, 22.0, 82).reshape(1, 1, 82, 1, 1), kind == 'space', True, True, True, 'bior1.3', 'zero', [list(FINE)], None,
                            image_size=40, frames=24, timesteps=1000, sampling_timesteps=250, loss_type='l2').to(DEV)
    return TrainStep(dif, lr=1e-4, betas=(0.9, 0.99), max_grad_norm=1.0, lr_schedule=multistep_lr, use_ema=True)


def bench_step(kind, batch, sims, steps, pack_ms):
    """(c)"""
    from wdno_amd.trainer import cycle_loader
    assert sims % batch == 0, '--sims must be a multiple of every --batch (the captured step takes full batches only)'
    root = tempfile.mkdtemp(prefix='wdno_bench_super_')
    try:
        write_files(root, kind, sims)
        sets = [Smoke_wave(root, 'bior1.3', 'zero', is_super_model=True, downsample_type=kind, N_downsample=0)]
        sets[0].n_simu = sims
        ts = build_step(kind, batch)
        ld = ResidentSuperSmokeLoader(sets, batch, DEV, num_workers=8)
        it = cycle_loader(ld)
        x = next(it)[0].clone()
        for _ in range(2):
            ts.step(x)
        ts.capture(x, warmup=1)

        def rate(next_batch, n):
            for _ in range(2):
                ts.step(next_batch())
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                ts.step(next_batch())
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n
        for _ in range(len(ld)):                           # the rest of epoch 1: every file into HBM
            next(it)
        assert len(ld.slot) == sims
        dt_tensor = [rate(lambda: x, steps)]
        dt_loader = [rate(lambda: next(it)[0], steps)]
        dt_tensor.append(rate(lambda: x, steps))
        dt_loader.append(rate(lambda: next(it)[0], steps))
        dl = cycle_loader(SuperDataLoader(sets, batch_size=batch, shuffle=True, pin_memory=True, num_workers=4))
        dt_ref = rate(lambda: next(dl)[0].to(DEV, non_blocking=True), steps)
        del dl
        t, l = min(dt_tensor), min(dt_loader)
        expect = t / (t + pack_ms * 1e-3)
        ratio = t / l
        ok = ratio >= expect - 0.01
        print(json.dumps(dict(what='super_step', kind=kind, batch=batch, simulations=sims, steps_per_window=steps,
                              resident_tensor_ms_per_step=[round(v * 1e3, 3) for v in dt_tensor], resident_loader_ms_per_step=[round(v * 1e3, 3) for v in dt_loader],
                              super_dataloader_4_workers_ms_per_step=round(dt_ref * 1e3, 3), pack_kernel_ms=round(pack_ms, 5),
                              loader_rate_over_tensor_rate=round(ratio, 4), expected_step_over_step_plus_pack=round(expect, 4), gate=round(expect - 0.01, 4),
                              gate_passed=bool(ok), super_dataloader_rate_over_tensor_rate=round(t / dt_ref, 4), resident_MB=round(ld.resident_bytes() / 1e6, 1))),
              flush=True)
        return ok
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--kind', nargs='+', default=['time', 'space'], choices=['time', 'space'])
    ap.add_argument('--batch', nargs='+', type=int, default=[6, 8])
    ap.add_argument('--sims', type=int, default=48)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--skip-step', action='store_true')
    a = ap.parse_args()
    good = True
    for kind in a.kind:
        for batch in a.batch:
            pack_ms = bench_kernel(kind, batch, a.sims)
            if not a.skip_step:
                good = bench_step(kind, batch, a.sims, a.steps, pack_ms) and good
    sys.exit(0 if good else 1)
