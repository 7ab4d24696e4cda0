"""Timings of the resident input pipeline of the Burgers super-resolution trainer on one GPU (profiles/burgers_super_loader.md), at the three real
levels: fine [2, 4, 41, 60] / [2, 4, 21, 30] / [2, 4, 11, 15] with the next-coarser level -> state [B, 17, 64 / 32 / 16, same].

  (a) kernel      wdno_pack_burgers_state for a batch drawn by an index list from `--samples` resident samples, against index_select on a resident
                  packed tensor (what ResidentTensorLoader would do with DiffusionDataset.x in HBM) and against the present per-level chain on
                  device tensors (gather, cat + pad, IDWT of both fields, 1-D DWT of two rows, division). Per Python call (host enqueue included)
                  and, for the kernel and the gather, per replay of 20 calls captured in one graph. Bytes read plus written per microsecond of the
                  kernel next to pack_smoke_state_kernel<0> on [8, 24, 42, 40, 40] in the same run: a yardstick, not a gate.
  (b) step        the full-width training step (Unet2D(dim=128, (1, 2, 4, 8), channels=17), graph replay) per level, fed by one resident state
                  tensor, by ResidentSuperBurgersLoader held to that level, and by SuperDataLoader on the level's dataset with the Trainer's default
                  workers. Gate: loader rate / tensor rate >= step / (step + kernel) - 0.01, all three terms from this run.
  (c) start-up    from the coefficient file to the first batch, with peak host (ru_maxrss) and device memory, each arm in a child process of its
                  own: the resident loader (one read, levels uploaded, first batch packed) against the parent's route (the file read and the packed
                  tensor built once per level dataset, first batch from SuperDataLoader without workers).
Prints one JSON line per measurement; exit status 1 when a gate fails. `--skip-step` / `--skip-startup` split the work into short runs."""
import argparse
import gc
import json
import os
import resource
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wdno_amd import tree_path  # noqa: E402

for _t in ('third_party', 'smoke', 'burgers'):
    sys.path.insert(0, tree_path(_t))
import ddpm_burgers.data_burgers_1d as DB  # noqa: E402
from wdno_amd.loader import ResidentSuperBurgersLoader  # noqa: E402

DEV = 'cuda'
WAVE, MODE = 'bior2.4', 'periodization'
LEVELS = [(41, 60), (21, 30), (11, 15), (6, 8)]
RESC = torch.tensor([10, 3, 3, 1, 21, 5, 5, 1, 10, 3, 3, 1, 21, 5, 5, 1, 10]).view(1, 17, 1, 1).float()


def ori_of(lvl):
    return [-(-81 // 2 ** lvl), -(-120 // 2 ** lvl)]


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


def _graph(fn):
    """ms per call replayed from 20 calls captured in one graph (median of 5 windows of 10 replays) and the windows' spread in percent."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(20):
            fn()
    w = sorted(_ev_time(g.replay, 10) / 20 for _ in range(5))
    return w[2], 100 * (w[-1] - w[0]) / w[2]


def synthetic_db(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    coef = [torch.randn(n, 2, 4, *s, generator=g) * 3 for s in LEVELS]
    return {'coef': coef, 'shape': [c.shape[2:] for c in coef], 'ori_shape': torch.Size((81, 120))}


def level_datasets(db, n_sets=3):
    return [DB.DiffusionDataset(db, preprocess=DB.get_wavelet_super_preprocess(rescaler=RESC, is_super_model=True, N_downsample=i, mode=MODE,
                                                                               wave_type=WAVE)) for i in range(n_sets)]


def bench_kernel(lvl, batch, samples):
    """(a). Returns the kernel's ms per batch (graph figure) for the gate of (b)."""
    from ddpm.data_2d import pack_smoke_gpu, _RESCALERS
    db = synthetic_db(samples, seed=1)
    fine, coarse = db['coef'][lvl].to(DEV), db['coef'][lvl + 1].to(DEV)
    pad, ori, r = 64 >> lvl, ori_of(lvl), RESC.to(DEV)
    idx = torch.randperm(samples, generator=torch.Generator().manual_seed(2))[:batch].to(DEV)
    kernel = lambda: DB.pack_burgers_gpu(fine, coarse, r, ori, idx, pad, pad, WAVE)
    chain = lambda: DB._pack_index(fine.index_select(0, idx), coarse.index_select(0, idx), r, ori, pad, pad, MODE, WAVE, True, True)
    packed = DB._pack_index(fine, coarse, r, ori, pad, pad, MODE, WAVE, True, True)              # DiffusionDataset.x of the level, in HBM
    gather = lambda: packed.index_select(0, idx)
    assert torch.equal(kernel(), chain()) and torch.equal(kernel(), gather())
    out = dict(what='pack_burgers_kernel', level=lvl, batch=batch, resident_samples=samples)
    for name, fn in (('kernel', kernel), ('gather', gather)):
        out[f'{name}_ms_per_call'] = round(_ev_time(fn, 20), 5)
        ms, spread = _graph(fn)
        out[f'{name}_ms_in_graph'], out[f'{name}_graph_spread_pct'] = round(ms, 5), round(spread, 1)
    out['chain_ms_per_call'] = round(_ev_time(chain, 20), 5)           # (host enqueue included: the chain allocates and copies between its launches)
    k_bytes = 4 * batch * (fine[0].numel() + coarse[0].numel() + 17 * pad * pad)
    out['kernel_bytes'], out['kernel_bytes_per_us'] = k_bytes, round(k_bytes / (out['kernel_ms_in_graph'] * 1e3), 1)
    out['gather_bytes_per_us'] = round(4 * batch * 2 * 17 * pad * pad / (out['gather_ms_in_graph'] * 1e3), 1)
    # the yardstick: the base smoke packing kernel on its bench shape, same graph method
    g = torch.Generator(device=DEV).manual_seed(1)
    s_coef, s_init = torch.randn(48, 5, 8, 18, 34, 34, device=DEV, generator=g), torch.randn(48, 4, 34, 34, device=DEV, generator=g)
    s_so, r42 = torch.rand(48, 2, 18, device=DEV, generator=g), torch.tensor(_RESCALERS['bior1.3'], dtype=torch.float32, device=DEV)
    s_idx = torch.arange(8, device=DEV) * 5
    b_ms, b_spread = _graph(lambda: pack_smoke_gpu(s_coef, s_init, s_so, r42, s_idx))
    b_bytes = 4 * 8 * (s_coef[0].numel() + s_init[0].numel() + s_so[0].numel() + 24 * 42 * 40 * 40)
    out.update(smoke_base_kernel_ms_in_graph=round(b_ms, 5), smoke_base_graph_spread_pct=round(b_spread, 1), smoke_base_bytes_per_us=round(b_bytes / (b_ms * 1e3), 1))
    print(json.dumps(out), flush=True)
    return out['kernel_ms_in_graph']


class _OneLevel:
    def __init__(self, lvl):
        self.lvl = lvl

    def randint(self, a, b):
        return self.lvl


def bench_step(batch, samples, steps, pack_ms, dim, groups=1):
    """(b)"""
    from ddpm_burgers.diffusion_1d import GaussianDiffusion
    from ddpm_burgers.unet import Unet2D
    from wdno_amd.trainer import TrainStep, cosine_annealing_lr, cycle_loader
    assert samples % batch == 0, '--samples must be a multiple of --batch (the captured step takes full batches only)'
    sets = level_datasets(synthetic_db(samples, seed=3))
    ld = ResidentSuperBurgersLoader(sets, batch, DEV)
    it = cycle_loader(ld)
    good = True
    for lvl in range(3):
        torch.manual_seed(0)
        net = Unet2D(dim=dim, dim_mults=(1, 2, 4, 8), channels=17, resnet_block_groups=groups)
        dif = GaussianDiffusion(net, seq_length=(64, 64), is_wavelet=True, pad_mode=MODE, wave_type=WAVE, padded_shape=[list(s) for s in LEVELS[:3]],
                                ori_shape=[ori_of(i) for i in range(3)], is_super_model=True, timesteps=1000, loss_layer_weight=RESC,
                                is_condition_pad=True, is_condition_u0=True, is_condition_uT=True).to(DEV)
        ts = TrainStep(dif, lr=1e-4, betas=(0.9, 0.99), max_grad_norm=1.0, lr_schedule=lambda b, s: cosine_annealing_lr(b, s, 10000, 0.0), use_ema=True)
        ld._rng = _OneLevel(lvl)
        x = next(it).clone()
        try:
            for _ in range(2):
                ts.step(x)
            ts.capture(x, warmup=1)
        except (RuntimeError, ValueError, AssertionError) as e:      # a kernel of the step that refuses the level's shape: reported, not timed
            print(json.dumps(dict(what='burgers_super_step', level=lvl, batch=batch, dim=dim, step_error=repr(e)[:300])), flush=True)
            continue

        def rate(next_batch, n):
            for _ in range(2):
                ts.step(next_batch())
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                ts.step(next_batch())
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n
        dt_tensor = [rate(lambda: x, steps)]
        dt_loader = [rate(lambda: next(it), steps)]
        dt_tensor.append(rate(lambda: x, steps))
        dt_loader.append(rate(lambda: next(it), steps))
        workers = min(os.cpu_count(), 16)
        t0 = time.perf_counter()
        dl = cycle_loader(DB.SuperDataLoader([sets[lvl]], batch_size=batch, shuffle=True, pin_memory=True, num_workers=workers))
        first = next(dl)
        t_first = time.perf_counter() - t0
        dt_ref = rate(lambda: next(dl).to(DEV, non_blocking=True), steps)
        del dl, first
        t, l = min(dt_tensor), min(dt_loader)
        expect, ratio = t / (t + pack_ms[lvl] * 1e-3), t / l
        ok = ratio >= expect - 0.01
        good = good and ok
        print(json.dumps(dict(what='burgers_super_step', level=lvl, batch=batch, dim=dim, samples=samples, steps_per_window=steps,
                              resident_tensor_ms_per_step=[round(v * 1e3, 3) for v in dt_tensor], resident_loader_ms_per_step=[round(v * 1e3, 3) for v in dt_loader],
                              super_dataloader_ms_per_step=round(dt_ref * 1e3, 3), super_dataloader_workers=workers,
                              super_dataloader_first_batch_s=round(t_first, 2), pack_kernel_ms=round(pack_ms[lvl], 5),
                              loader_rate_over_tensor_rate=round(ratio, 4), expected_step_over_step_plus_pack=round(expect, 4), gate=round(expect - 0.01, 4),
                              gate_passed=bool(ok), super_dataloader_rate_over_tensor_rate=round(t / dt_ref, 4))), flush=True)
        del ts, net, dif
        gc.collect()
    return good


def startup_arm(arm, path, batch):
    """(c), one arm in this (fresh) process."""
    torch.cuda.init()
    torch.zeros(1, device=DEV)
    torch.cuda.synchronize()
    rss0 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    pre = lambda i: DB.get_wavelet_super_preprocess(rescaler=RESC, is_super_model=True, N_downsample=i, mode=MODE, wave_type=WAVE)
    if arm == 'resident':
        sets = [DB.DiffusionDataset(path, preprocess=pre(i)) for i in range(3)]
        ld = ResidentSuperBurgersLoader(sets, batch, DEV)
        (x,) = list(ld)
    else:                                  # the parent's route: a read and an eager packed tensor per level dataset
        sets = []
        for i in range(3):
            ds = DB.DiffusionDataset(torch.load(path, weights_only=False), preprocess=pre(i))
            ds.x
            sets.append(ds)
        x = next(iter(DB.SuperDataLoader(sets, batch_size=batch, shuffle=True, pin_memory=True, num_workers=0))).to(DEV)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps(dict(what='burgers_super_startup', arm=arm, samples=len(sets[0]), first_batch=list(x.shape), seconds_to_first_batch=round(dt, 3),
                          peak_host_rss_MB=round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024, 1), host_rss_before_MB=round(rss0 / 1024, 1),
                          peak_device_MB=round(torch.cuda.max_memory_allocated() / 1e6, 1))), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--samples', type=int, default=256)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--dim', type=int, default=128)
    ap.add_argument('--startup-samples', type=int, default=4000)
    ap.add_argument('--skip-step', action='store_true')
    ap.add_argument('--skip-startup', action='store_true')
    ap.add_argument('--startup-arm', choices=['resident', 'parent'])
    ap.add_argument('--file')
    a = ap.parse_args()
    if a.startup_arm:
        startup_arm(a.startup_arm, a.file, a.batch)
        sys.exit(0)
    pack_ms = [bench_kernel(lvl, a.batch, a.samples) for lvl in range(3)]
    good = True
    if not a.skip_step:
        good = bench_step(a.batch, a.samples, a.steps, pack_ms, a.dim)
    if not a.skip_startup:
        with tempfile.TemporaryDirectory(prefix='wdno_bench_burgers_') as root:
            path = os.path.join(root, 'coef_bior2.4_periodization_super')
            torch.save(synthetic_db(a.startup_samples, seed=5), path)
            for arm in ('resident', 'parent'):                    # a fresh child each: ru_maxrss and the allocator's peak are per process
                subprocess.run([sys.executable, os.path.abspath(__file__), '--startup-arm', arm, '--file', path, '--batch', str(a.batch)], check=True, timeout=600)
    sys.exit(0 if good else 1)
