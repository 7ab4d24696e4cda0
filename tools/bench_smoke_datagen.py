"""Time the smoke data-set generator (wdno_amd.smoke_datagen.generate with the seeded noise source, one launch of csrc/smoke_datagen.hip:
257 frames x up to 500 CG iterations per scene) at batch 1, 50 and 256 against the control-evaluation solver (wdno_amd.smoke_solver.solve,
256 frames) at the same batch in the same run, the two alternating; then write_dataset end to end, with the file writes.

Device events around each call after one warm-up call of each; the median of --reps calls (the method of tools/bench_smoke_solver.py).
The solver writes its last frame only (frames=[255]); the generator writes its 33 records of 64 x 64. write_dataset is timed on the
wall clock (it ends with the last file on disk) for --scenes scenes into --out (default: a temporary directory) and reported in scenes / s
and against the reference's wall time per scene (tests/golden/ref_smoke_datagen_manifest.json: reference_wall_s of the 256-frame cases).
One JSON line per measurement.

    python tools/bench_smoke_datagen.py [--reps 5] [--scenes 512] [--out DIR] [--dtype float64]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bench_smoke_solver import inputs  # noqa: E402
from wdno_amd import smoke_datagen as GEN, smoke_solver as W  # noqa: E402

BATCHES = (1, 50, 256)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--scenes', type=int, default=512)
    ap.add_argument('--out', default=None)
    ap.add_argument('--dtype', choices=('float64', 'float32'), default='float64')
    ap.add_argument('--seed', type=int, default=0)
    a = ap.parse_args()
    for B in BATCHES:
        scenes = GEN.sample_scenes(range(B), a.seed, 256)
        d0, c1, c2 = inputs(B)
        gen = lambda: GEN.generate(scenes, seed=a.seed)
        sol = lambda: W.solve(d0, c1, c2, frames=[255])
        gen(); sol()
        torch.cuda.synchronize()
        g_ms, s_ms = [], []
        for _ in range(a.reps):
            g_ms.append(timed(gen))
            s_ms.append(timed(sol))
        g, s = statistics.median(g_ms), statistics.median(s_ms)
        print(json.dumps(dict(batch=B, threads=W.DEFAULT_THREADS, generate_median_ms=round(g, 2), solve_median_ms=round(s, 2),
                              generate_over_solve=round(g / s, 4), generate_calls_ms=[round(x, 2) for x in g_ms],
                              solve_calls_ms=[round(x, 2) for x in s_ms], scenes_per_s=round(B / g * 1e3, 1))), flush=True)
        del d0, c1, c2
        torch.cuda.empty_cache()
    if a.scenes > 0:
        out = a.out or tempfile.mkdtemp(prefix='smoke_datagen_bench_')
        try:
            GEN.write_dataset(out, 'train', range(2), a.seed, dtype=np.dtype(a.dtype).type)          # warm-up: library, pool, pinned memory
            t0 = time.perf_counter()
            GEN.write_dataset(out, 'train', range(a.scenes), a.seed, dtype=np.dtype(a.dtype).type)
            wall = time.perf_counter() - t0
            size = sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(out) for f in fs)
        finally:
            if a.out is None:
                shutil.rmtree(out, ignore_errors=True)
        rec = dict(write_dataset_scenes=a.scenes, dtype=a.dtype, wall_s=round(wall, 2), scenes_per_s=round(a.scenes / wall, 1),
                   bytes_per_scene=size // max(a.scenes, 1))
        try:
            with open(os.path.join(ROOT, 'tests', 'golden', 'ref_smoke_datagen_manifest.json')) as f:
                cases = json.load(f)['cases']
            ref = statistics.mean(c['reference_wall_s'] for c in cases.values() if c['scenelength'] == 256)
            rec.update(reference_wall_s_per_scene=round(ref, 1), speedup_vs_one_reference_process=round(ref * a.scenes / wall))
        except OSError:
            pass
        print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
