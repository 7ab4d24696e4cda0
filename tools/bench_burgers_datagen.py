"""Time one 800-trajectory batch of the Burgers data set at the reference's shape (s = 1920, t = 1280, T = 8, nt = 80, nx = 120: the
constants of generate_data_burgers_equation and the 80 / 120 data_burgers_1d.py reads) two ways, alternating after a warm-up of both:

  (a) the dense path: make_data_varying_f's expressions restated here (with their `.repeat`s) on the GPU -> f [800, 1280, 1920] (7.9 GB),
      then burgers_solver.solve (csrc/burgers.hip), then the two slices;
  (b) burgers_datagen.draw + burgers_datagen.generate (csrc/burgers_datagen.hip): two tables of 102 KB per trajectory, one launch.

Device events around each part, the median and the spread of --reps rounds, torch.cuda.max_memory_allocated of each path, and whether the two
paths return the same bits from the same seed. If (a) does not fit in memory that is reported as its result and its solve is timed alone on
a dense f built in slices from the tables. --sweep times every supported (W, P) of the table kernel at N = 800 (median of 3).
One JSON line per measurement. Kernel times come from a run of its own under rocprofv3 --kernel-trace --stats.

    python tools/bench_burgers_datagen.py [--reps 5] [--sweep] [--N 800]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wdno_amd import burgers_datagen as D, burgers_solver as B  # noqa: E402

S, T_F, T, NT, NX, VISC = 1920, 1280, 8.0, 80, 120, 0.01
SEED = 0


def dense_draw(N, s, t, device, amp_compensate=2):
    """make_data_varying_f (generate_burgers.py:207-275, alpha = 1) restated: the same calls, the same `.repeat` temporaries."""
    x = torch.linspace(1.0 / (s + 1), 1.0 - 1.0 / (s + 1), s).to(device)
    ts = torch.linspace(1.0 / (t + 1), 1.0 - 1.0 / (t + 1), t).to(device)
    loc1 = torch.rand(N, 1, device=device) * 0.2 + 0.2
    amp1 = torch.rand(N, 1, device=device) * 2
    sig1 = torch.rand(N, 1, device=device) * 0.1 + 0.05
    gauss1 = amp1 * torch.exp(-0.5 * (x.view(1, -1) - loc1) ** 2 / sig1 ** 2)
    loc2 = torch.rand(N, 1, device=device) * 0.2 + 0.6
    amp2 = torch.rand(N, 1, device=device) * 2 - 2
    sig2 = torch.rand(N, 1, device=device) * 0.1 + 0.05
    gauss2 = amp2 * torch.exp(-0.5 * (x.view(1, -1) - loc2) ** 2 / sig2 ** 2)
    u0 = gauss1 + gauss2

    def rand_f(is_rand_amp=True):
        if is_rand_amp:
            amp = torch.randint(2, (N, 1, 1), device=device).float() * (torch.rand(N, 1, 1, device=device) * 3 - 1.5)
        else:
            amp = (torch.rand(N, 1, 1, device=device) * 3 - 1.5)
        amp = amp.repeat(1, t, s)
        loc = torch.rand(N, 1, 1, device=device)
        sig = torch.rand(N, 1, 1, device=device) * 0.3 + 0.1
        exp_space = torch.exp(-0.5 * (x.view(1, 1, -1).repeat(N, t, 1) - loc) ** 2 / sig ** 2)
        loc = torch.rand(N, 1, 1, device=device)
        sig = torch.rand(N, 1, 1, device=device) * 0.3 + 0.1
        exp_time = amp_compensate * torch.exp(-0.5 * (ts.view(1, -1, 1).repeat(N, 1, s) - loc) ** 2 / sig ** 2)
        return amp * exp_space * exp_time
    f = rand_f(is_rand_amp=False)
    for _ in range(7):
        f += rand_f(is_rand_amp=True)
    return u0, f.to(torch.float32)


class Parts:
    """Device events at the boundaries of a path's parts: times(names) after a synchronise."""
    def __init__(self):
        self.ev = []

    def mark(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.ev.append(e)

    def times(self, names):
        torch.cuda.synchronize()
        return {n: self.ev[i].elapsed_time(self.ev[i + 1]) for i, n in enumerate(names)}


def path_a(N):
    p = Parts()
    torch.manual_seed(SEED)
    p.mark()
    u0, f = dense_draw(N, S, T_F, 'cuda')
    p.mark()
    traj = B.solve(u0, f, VISC, T, num_t=NT, s=S)
    p.mark()
    out = traj[:, :, ::int(S / NX)].contiguous(), f[:, ::int(T_F / NT), ::int(S / NX)].contiguous()
    p.mark()
    return out, p.times(('forcing', 'solve', 'slices'))


def path_b(N, config=None):
    p = Parts()
    torch.manual_seed(SEED)
    p.mark()
    u0, AX, TT = D.draw(N, S, T_F, 'cuda')
    p.mark()
    out = D.generate(u0, AX, TT, T, NT, NX, NT, config=config)
    p.mark()
    return out, p.times(('draw', 'generate'))


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated() - base


def summary(rows):
    return {k: dict(median_ms=round(statistics.median(r[k] for r in rows), 3), min_ms=round(min(r[k] for r in rows), 3),
                    max_ms=round(max(r[k] for r in rows), 3)) for k in rows[0]}


def solve_alone(N, reps):
    """(a)'s solve on a dense f built in slices from the tables, alternated with generate on the same tables."""
    torch.manual_seed(SEED)
    u0, AX, TT = D.draw(N, S, T_F, 'cuda')
    f = torch.empty(N, T_F, S, device='cuda')
    for i in range(0, N, 50):
        f[i:i + 50] = D.dense_forcing(AX[i:i + 50], TT[i:i + 50])
    rows = []
    for r in range(reps + 1):
        p = Parts()
        p.mark()
        a = B.solve(u0, f, VISC, T, num_t=NT, s=S)
        p.mark()
        b = D.generate(u0, AX, TT, T, NT, NX, NT)
        p.mark()
        if r:
            rows.append(p.times(('solve_kernel_call', 'generate_kernel_call')))
        else:
            torch.cuda.synchronize()
            same = bool(torch.equal(a[:, :, ::int(S / NX)], b[0]) and torch.equal(f[:, ::int(T_F / NT), ::int(S / NX)], b[1]))
        del a, b
    return summary(rows), same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--N', type=int, default=800)
    ap.add_argument('--sweep', action='store_true')
    a = ap.parse_args()
    N = a.N
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    pl = D.plan(N, S, T_F, T, NT, NX, NT, cu_count=cus)
    head = dict(N=N, s=S, t=T_F, T=T, nt=NT, nx=NX, steps=pl['steps'], f_time=pl['f_time'], config=[pl['waves'], pl['points']])

    (out_b, _), peak_b = peak_of(lambda: path_b(N))                       # warm-up of (b), and its memory peak
    try:
        (out_a, _), peak_a = peak_of(lambda: path_a(N))                   # warm-up of (a), and its memory peak
        fits = True
    except torch.cuda.OutOfMemoryError as e:
        fits, out_a, peak_a = False, None, None
        print(json.dumps(dict(head, path='a', result='does not fit in memory', error=str(e)[:200])), flush=True)
    if fits:
        same = bool(torch.equal(out_a[0], out_b[0]) and torch.equal(out_a[1], out_b[1]))
        del out_a
    del out_b
    torch.cuda.empty_cache()
    rows_a, rows_b = [], []
    for _ in range(a.reps):                                                # alternating
        if fits:
            out, t = path_a(N)
            t['total'] = sum(t.values())
            rows_a.append(t)
            del out
            torch.cuda.empty_cache()
        out, t = path_b(N)
        t['total'] = sum(t.values())
        rows_b.append(t)
        del out
    if fits:
        print(json.dumps(dict(head, path='a', peak_bytes=peak_a, same_bits_as_b=same, **summary(rows_a))), flush=True)
    print(json.dumps(dict(head, path='b', peak_bytes=peak_b, **summary(rows_b))), flush=True)
    torch.cuda.empty_cache()
    alone, same_k = solve_alone(N, a.reps)
    print(json.dumps(dict(head, path='kernels alternated on one dense f', same_bits=same_k, **alone)), flush=True)
    torch.cuda.empty_cache()
    if a.sweep:
        torch.manual_seed(SEED)
        u0, AX, TT = D.draw(N, S, T_F, 'cuda')
        for cfg in B.configs(S):
            ms = []
            for r in range(4):
                p = Parts()
                p.mark()
                D.generate(u0, AX, TT, T, NT, NX, NT, config=cfg)
                p.mark()
                if r:
                    ms.append(p.times(('g',))['g'])
                else:
                    torch.cuda.synchronize()
            m = statistics.median(ms)
            print(json.dumps(dict(N=N, sweep=list(cfg), median_ms=round(m, 3), cycles_per_step_at_2400MHz=round(m * 1e-3 * 2.4e9 / pl['steps']))),
                  flush=True)


if __name__ == '__main__':
    main()
