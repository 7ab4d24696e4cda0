"""Timings of the Burgers evaluation driver's two kernels and of one whole evaluation batch on one GPU (profiles/burgers_eval.md):

  --reconstruct   wdno_amd.burgers.reconstruct.reconstruct (one launch) against the chain it replaces (x * RESCALER -> tensor_to_coef ->
                  wdno_amd.wavelets.DWTInverse -> the two crops) at the evaluation shape, x [B, 9, 64, 64], block (41, 60), fields (81, 120).
  --score         wdno_amd.burgers.score.score (one launch, one device-to-host copy) against mse_deviation + the two torch metric calls with
                  the .cpu() copies diffuse_2dconv makes of their results.
                  Both: device events around `--iters` back-to-back calls per window, 5 windows, the arms alternating inside each window,
                  every arm run once untimed, one process; spread = (max - min) / median. Kernel launches of one call of each arm are
                  counted with torch.profiler.
  --batch-split   one whole evaluation batch (1000 guided DDPM steps of the full-size U-Net with random weights, then reconstruction,
                  solver and scoring) split into sampling / solver / everything else, and get_target's five calls of a batch with the
                  file held against five reads (a synthetic test file, 4 x up-sampled: u [50, 321, 480]).
Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wdno_amd import tree_path  # noqa: E402

for _t in ('third_party', 'burgers'):
    sys.path.insert(0, tree_path(_t))
from wave_trans import tensor_to_coef  # noqa: E402
from wdno_amd import wavelets as W  # noqa: E402
from wdno_amd.burgers.reconstruct import reconstruct  # noqa: E402
from wdno_amd.burgers import score as S  # noqa: E402

SHAPE, ORI = (41, 60), (81, 120)
RESCALER = [10, 3, 3, 1, 21, 5, 5, 1, 10]


def chain(x, resc):
    """diffuse_2dconv's wavelet branch (eval_ddpm_burgers.py:185-195) on the existing operators."""
    xs = x * resc
    yl, yh = tensor_to_coef(xs, SHAPE)
    u_f = W.DWTInverse(mode='periodization', wave='bior2.4')((yl.contiguous(), [v.contiguous() for v in yh]))[:, :, :ORI[0], :ORI[1]]
    return u_f[:, 0], u_f[:, 1, :ORI[0] - 1]


def torch_metrics(u, f, x_gt, ut, wf):
    """What diffuse_2dconv runs between the solver and its return (eval_ddpm_burgers.py:220-237) on this tree's plain-torch metric."""
    from ddpm_burgers.test_util import metric, mse_deviation
    sub = int(x_gt.shape[-1] / u.shape[-1])
    ddpm_mse = mse_deviation(u[:, 1:], x_gt[:, 1:, ::sub]).cpu()
    u_repeat = u.unsqueeze(-1).expand(*u.shape, sub).reshape(u.shape[0], u.shape[1], u.shape[2] * sub)
    jd, _, _ = metric(ut, f, 0, wf=wf, report_all=True, u=u_repeat, evaluate=True)
    ja, en, tj = metric(ut, f, 0, wf=wf, report_all=True, u=x_gt, evaluate=True)
    return ddpm_mse, np.array([v.cpu().numpy() for v in jd]), np.array([v.cpu().numpy() for v in ja]), en.cpu().numpy(), tj.cpu().numpy()


def _window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _launches(fn):
    """Kernel launches of one call (None when the profiler is not available)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith('CUDA') and 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower())
    except Exception as exc:          # noqa: BLE001
        print(f'(launch count unavailable: {exc})', file=sys.stderr)
        return None


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
    out['ratio_chain_over_kernel'] = out['chain']['median_ms'] / out['kernel']['median_ms']
    print(json.dumps(out), flush=True)


def _state(batch):
    gen = torch.Generator(device='cuda').manual_seed(1)
    x = torch.randn(batch, 9, 64, 64, device='cuda', generator=gen) * 0.4
    return x, torch.tensor(RESCALER, dtype=torch.float32, device='cuda').reshape(1, 9, 1, 1)


def bench_reconstruct(batch, iters):
    x, resc = _state(batch)
    (a, b), (c, d) = reconstruct(x, SHAPE, ORI, resc), chain(x, resc)
    rel = max(float((a - c).abs().max() / c.abs().max()), float((b - d).abs().max() / d.abs().max()))
    _arms('reconstruct', {'kernel': lambda: reconstruct(x, SHAPE, ORI, resc), 'chain': lambda: chain(x, resc)}, iters, batch=batch,
          kernel_vs_chain_relmax=rel)


def bench_score(batch, iters, wf=0.03):
    x, resc = _state(batch)
    u, f = reconstruct(x, SHAPE, ORI, resc)
    gen = torch.Generator(device='cuda').manual_seed(2)
    x_gt = torch.randn(batch, ORI[0], ORI[1], device='cuda', generator=gen) * 0.3
    ut = torch.randn(batch, ORI[0], ORI[1], device='cuda', generator=gen) * 0.3
    a, b = S.score(u, f, x_gt, ut, wf), torch_metrics(u, f, x_gt, ut, wf)
    rel = max(float(np.abs(v - np.asarray(w, dtype=np.float64)).max() / np.abs(v).max()) for v, w in zip(a, (b[0].numpy(),) + b[1:]))
    _arms('score', {'kernel': lambda: S.score(u, f, x_gt, ut, wf), 'chain': lambda: torch_metrics(u, f, x_gt, ut, wf)}, iters, batch=batch,
          kernel_vs_chain_relmax=rel)


def bench_batch(batch):
    import eval_ddpm_burgers as E
    from ddpm_burgers import test_util as TU
    args = E.build_parser().parse_args(['--exp_id', 'bench', '--is_condition_u0', 'True', '--is_condition_uT', 'True'])
    resc = E.rescaler_table(args)
    timers = {'sampling': 0.0, 'solver': 0.0}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            os.makedirs('data/1d_super')
            gen = torch.Generator().manual_seed(3)
            torch.save({'u': 0.3 * torch.randn(batch, 321, 480, generator=gen), 'f': 0.3 * torch.randn(batch, 320, 480, generator=gen)}, 'data/1d_super/test')
            torch.manual_seed(0)
            ddpm = TU.get_2d_ddpm(list(SHAPE), list(ORI), args, resc, is_super_model=False).cuda()
            E.load_2dconv_base_model = lambda model_i, a, r: ddpm
            real_sample, real_solve = ddpm.sample, E.burgers_numeric_solve_free

            def timed(key, fn):
                def run(*a, **k):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = fn(*a, **k)
                    torch.cuda.synchronize()
                    timers[key] += time.perf_counter() - t0
                    return out
                return run
            ddpm.sample = timed('sampling', real_sample)
            E.burgers_numeric_solve_free = timed('solver', real_solve)
            out = dict(what='batch', batch=batch, steps=ddpm.num_timesteps)
            for run in ('first', 'second'):          # the first call captures the guided step and reads the file; the second is the steady state
                timers.update(sampling=0.0, solver=0.0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                E.evaluate('bench', '', args, Ntest=batch, batch_size=batch, wu=0.5, wf=0.01, RESCALER=resc)
                torch.cuda.synchronize()
                total = time.perf_counter() - t0
                out[run] = dict(total_s=total, sampling_s=timers['sampling'], solver_s=timers['solver'], rest_s=total - timers['sampling'] - timers['solver'])
            # get_target: the five calls of a batch (eval_ddpm_burgers.py:278-295) with the file held, and re-read every time
            idx = list(range(batch))

            def five():
                TU.get_target(args, is_wave=False, target_i=idx, N_upsample=0, dataset='1d')
                TU.get_target(args, is_wave=True, target_i=idx, dataset='1d')
                TU.get_target(args, f=True, is_wave=True, target_i=idx, dataset='1d')
                TU.get_target(args, is_wave=False, target_i=idx, dataset='1d')
                TU.get_target(args, is_wave=False, target_i=idx, N_upsample=0, dataset='1d')
                torch.cuda.synchronize()

            def five_reads():
                for call in (lambda: TU.get_target(args, is_wave=False, target_i=idx, N_upsample=0, dataset='1d'),
                             lambda: TU.get_target(args, is_wave=True, target_i=idx, dataset='1d'),
                             lambda: TU.get_target(args, f=True, is_wave=True, target_i=idx, dataset='1d'),
                             lambda: TU.get_target(args, is_wave=False, target_i=idx, dataset='1d'),
                             lambda: TU.get_target(args, is_wave=False, target_i=idx, N_upsample=0, dataset='1d')):
                    TU._files.clear()
                    TU._views.clear()
                    call()
                torch.cuda.synchronize()
            for name, fn in (('get_target_held', five), ('get_target_five_reads', five_reads)):
                fn()
                ts = []
                for _ in range(20):
                    t0 = time.perf_counter()
                    fn()
                    ts.append(1e3 * (time.perf_counter() - t0))
                out[name] = dict(median_ms=float(np.median(ts)), spread_pct=100 * (max(ts) - min(ts)) / float(np.median(ts)))
            print(json.dumps(out), flush=True)
        finally:
            os.chdir(cwd)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reconstruct', action='store_true')
    ap.add_argument('--score', action='store_true')
    ap.add_argument('--batch-split', action='store_true')
    ap.add_argument('--batch', type=int, default=50)
    ap.add_argument('--iters', type=int, default=50)
    a = ap.parse_args()
    if a.reconstruct:
        bench_reconstruct(a.batch, a.iters)
    if a.score:
        bench_score(a.batch, a.iters)
    if a.batch_split:
        bench_batch(a.batch)
