"""Timings of the smoke inference pipeline's two kernels on one GPU (profiles/smoke_inference.md):

  --reconstruct   wdno_amd.smoke.reconstruct.reconstruct (one launch) against the chain it replaces (x * RESCALER -> tensor_to_coef ->
                  wavelets.waverec3 -> crop / permute -> the smoke-out means and 1-D IDWT -> expand -> cat) at the inference shape, state
                  [B, 24, 42, 40, 40], block (18, 34, 34), fields (32, 64, 64). Device events around `--iters` back-to-back calls per
                  window, 5 windows, the arms alternating inside each window, every arm run once untimed, one process;
                  spread = (max - min) / median.
  --score         peak device memory (torch.cuda.max_memory_allocated) and time of score_controls against evaluate_controls + the host
                  metrics, on `--batch` copies of a smooth control (the solver fixture's case `mid`).
  --once          a single reconstruct call (for a kernel trace's launch count), `--once-chain` the chain once.
Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wdno_amd import tree_path  # noqa: E402

for _t in ('third_party', 'smoke'):
    sys.path.insert(0, tree_path(_t))
from wave_trans_2d import tensor_to_coef  # noqa: E402
from wdno_amd import wavelets as W  # noqa: E402
from wdno_amd.smoke.reconstruct import reconstruct  # noqa: E402

SHAPE, ORI = (18, 34, 34), (32, 64, 64)


def chain(x, resc):
    """run_base_model's wavelet branch (inference_2d.py:137-152) on the existing operators: what bench.py's sr_leg times as idwt_reconstruction_ms."""
    wave_output = x * resc
    coef = tensor_to_coef(wave_output[:, :, :-2].permute(0, 2, 1, 3, 4), SHAPE)
    rec = W.waverec3([coef[0].contiguous(), {k: v.contiguous() for k, v in coef[1].items()}], 'bior1.3', 'zero')
    ori_output = rec[:, :ORI[0], :ORI[1], :ORI[2]].reshape(-1, 5, *ORI).permute(0, 2, 1, 3, 4)
    lo = wave_output[:, :SHAPE[0], -1, :20].mean((-2, -1)).unsqueeze(1)
    hi = wave_output[:, :SHAPE[0], -1, 20:].mean((-2, -1)).unsqueeze(1)
    smoke_out = W.DWT1DInverse(mode='zero', wave='bior1.3')((lo.contiguous(), [hi.contiguous()]))[:, 0]
    smoke_out = smoke_out[:, :ORI[0]].reshape(smoke_out.shape[0], ORI[0], 1, 1, 1).expand(-1, -1, -1, ORI[1], ORI[2])
    return torch.cat((ori_output, smoke_out), dim=2)


def _inputs(batch):
    gen = torch.Generator(device='cuda').manual_seed(1)
    x = torch.randn(batch, 24, 42, 40, 40, device='cuda', generator=gen) * 0.4
    return x, torch.linspace(1.0, 9.0, 42, device='cuda').reshape(1, 1, 42, 1, 1)


def _window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def bench_reconstruct(batch, iters):
    x, resc = _inputs(batch)
    arms = {'kernel': lambda: reconstruct(x, SHAPE, ORI, resc), 'chain': lambda: chain(x, resc)}
    a, b = arms['kernel'](), arms['chain']()
    rel = float((a - b).abs().max() / b.abs().max())
    t = {k: [] for k in arms}
    for _ in range(5):
        for k, fn in arms.items():
            t[k].append(_window(fn, iters))
    out = dict(what='reconstruct', batch=batch, iters=iters, kernel_vs_chain_relmax=rel)
    for k, v in t.items():
        med = float(np.median(v))
        out[k] = dict(median_ms=med, spread_pct=100 * (max(v) - min(v)) / med, windows_ms=[round(w, 4) for w in v])
    out['ratio_chain_over_kernel'] = out['chain']['median_ms'] / out['kernel']['median_ms']
    print(json.dumps(out), flush=True)


def bench_score(batch, w_energy=0.7):
    from tests import smoke_solver_ref as SR
    from tests.smoke_inference_inputs import metrics_fp64
    from wdno_amd.smoke.score import score_controls
    from wdno_amd.smoke_solver import evaluate_controls
    arrays, man = SR.load_golden()
    d0, c1, c2 = (torch.from_numpy(a).cuda() for a in SR.case_inputs(arrays, man, 'mid'))
    pred = 0.3 * torch.randn(batch, 32, 6, 64, 64, device='cuda', generator=torch.Generator(device='cuda').manual_seed(2))
    pred[:, :, 3], pred[:, :, 4] = c1, c2
    data = torch.zeros(batch, 256, 6, 64, 64, device='cuda')
    data[:, 0, 0] = d0
    out = dict(what='score', batch=batch)
    for arm in ('score_controls', 'evaluate_controls'):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        if arm == 'score_controls':
            r = score_controls(pred, data, w_energy)
        else:
            full = evaluate_controls(pred, data)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            p = pred.clone()
            p[:, :, 3:5, 8:56, 8:56] = 0
            r = metrics_fp64(p.cpu().numpy(), full[:, ::8, :, ::2, ::2].cpu().numpy(), w_energy)
            out['evaluate_controls_solve_s'] = t1 - t0
            del full
        torch.cuda.synchronize()
        out[arm] = dict(seconds=time.perf_counter() - t0, peak_bytes_above_inputs=torch.cuda.max_memory_allocated() - base,
                        J_total_mean=float(np.mean(r['J_total'])), mse_mean=float(np.mean(r['mse'])))
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reconstruct', action='store_true')
    ap.add_argument('--score', action='store_true')
    ap.add_argument('--once', action='store_true')
    ap.add_argument('--once-chain', action='store_true')
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--iters', type=int, default=200)
    a = ap.parse_args()
    if a.once or a.once_chain:
        x, resc = _inputs(a.batch)
        (chain if a.once_chain else (lambda x, r: reconstruct(x, SHAPE, ORI, r)))(x, resc)
        torch.cuda.synchronize()
    if a.reconstruct:
        bench_reconstruct(a.batch, a.iters)
    if a.score:
        bench_score(a.batch)
