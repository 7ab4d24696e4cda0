"""bench.py's plain run -- the main line only: set up, warm up, the timed steps, the JSON line -- and --dump-outputs, what the last timed
step computed, written for output-by-output comparisons of two builds. The side legs, the roofline step and the CPU baseline run with --full
(tests/test_gpu_bench_multirank.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, 'bench.py')


def test_bench_declares_full_and_dump_outputs_and_refuses_zero_steps():
    r = subprocess.run([sys.executable, BENCH, '--help'], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert '--full' in r.stdout and '--dump-outputs' in r.stdout
    r = subprocess.run([sys.executable, BENCH, '--steps', '0'], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and '--steps' in r.stderr and '{"metric"' not in r.stdout


@pytest.mark.gpu
def test_plain_run_is_the_main_line_and_dumps_the_last_step(tmp_path):
    """Two plain runs with the same arguments: the line holds the main measurement and nothing that --full adds, --steps is the number of
    timed steps, and the dumped arrays (float32 / float64, <= 64 MB) are the same in both runs -- same inputs, weights and draws."""
    runs = []
    for i in range(2):
        d = tmp_path / f'run{i}'
        r = subprocess.run([sys.executable, BENCH, '--gpus', '1', '--steps', '3', '--warmup', '1', '--dump-outputs', str(d)], cwd=ROOT,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
        assert len(lines) == 1, r.stdout[-2000:]
        out = json.loads(lines[0])
        assert out['steps'] == 3 and out['warmup'] == 1 and out['full'] is False
        assert out['unit'] == 'steps/s' and out['higher_is_better'] is True and out['dtype'] == 'f32'
        assert out['ms_per_step'] > 0 and abs(out['value'] - 1e3 / out['ms_per_step']) <= 0.01 * out['value']
        assert out['roofline'] is None and out['cpu_baseline'] is None
        assert not {'sampling', 'sr_sampling', 'dwt', 'burgers', 'fields_pipeline', 'loader', 'skipped_legs', 'error'} & out.keys()
        names = sorted(os.listdir(d))
        assert names == ['ema_sample.npy', 'grad_norm.npy', 'grads_sample.npy', 'loss.npy', 'params_sample.npy', 'sample_index.npy'], names
        arrays = {n[:-4]: np.load(d / n) for n in names}
        assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
        assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrays.values())
        assert float(arrays['loss']) == np.float32(out['final_loss']) and float(arrays['grad_norm']) > 0
        idx = arrays['sample_index']
        assert idx.shape == (1 << 20,) and np.all(np.diff(idx) > 0) and idx[0] >= 0
        assert arrays['params_sample'].shape == arrays['grads_sample'].shape == arrays['ema_sample'].shape == idx.shape
        assert np.abs(arrays['grads_sample']).max() > 0
        runs.append(arrays)
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k
