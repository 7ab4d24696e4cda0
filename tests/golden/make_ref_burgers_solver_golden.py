"""Golden vectors for the Burgers control-evaluation solver, burgers_numeric_solve_free
(burgers/ddpm_burgers/generate_burgers.py:104-204), by importing the reference.

Build-container only (needs /root/reference):   python tests/golden/make_ref_burgers_solver_golden.py
Writes tests/golden/ref_burgers_solver{,_b,_c}.npz and ref_burgers_solver_manifest.json -- data only: inputs, what the reference
returned, the `steps record_time f_time` line it printed, the exception class of each error case and its signature.

Beside the reference's fp32 output every case carries an fp64 evaluation of the same chain on the same fp32 inputs and fp32-rounded
constants (the convention of tests/arbiter.py), written here independently with slicing. It is stored as `<case>/exact_d` =
float32(exact - reference): the exact value is `ref.double() + exact_d.double()` to ~1e-7 of the difference, at half the bytes of a
float64 array (each committed file stays under 1 MiB). Before anything is written, the slicing form run in fp32 is checked against the
reference's own fp32 output (rel-L2 <= 1e-5), which pins it to the reference's operator.

Case A (the evaluation call, 614 400 steps) dominates the run time: the reference's loop costs ~3 ms a step there, ~40 CPU minutes in all.
"""
import contextlib
import inspect
import io
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_ref_golden as M  # noqa: E402

M.install_stubs()
from ddpm_burgers.generate_burgers import burgers_numeric_solve_free as ref_solve, make_data_varying_f  # noqa: E402

DT = 1 / 76800
VISC = 0.01


def sliced_solve(u0, f, visc, T, num_t, dt, s, dtype):
    """The reference's update restated with slices: ghosts are zero, interior point i sees u[i-1], u[i], u[i+1].
    fp32 inputs, fp32-rounded constants (generate_burgers.py:163-165), arithmetic in `dtype`. Returns [N, num_t + 1, s]."""
    N, Nt_f = u0.shape[0], f.shape[1]
    u = F.interpolate(u0.to(dtype)[:, None], size=s, mode='linear', align_corners=False)[:, 0]
    fi = F.interpolate(f.to(dtype), size=s, mode='linear', align_corners=False)
    dx = 1.0 / (s + 1)
    c = float(np.float32(1.0 / (2 * dx)))
    d = float(np.float32(visc * 1.0 / dx ** 2))
    dm = float(np.float32(visc * -2.0 / dx ** 2))
    dt32 = float(np.float32(dt))
    steps = math.ceil(T / dt)
    record_time, f_time = math.floor(steps / num_t), math.floor(steps / Nt_f)
    out = torch.zeros(N, num_t + 1, s, dtype=dtype)
    out[:, 0] = u
    up = torch.zeros(N, s + 2, dtype=dtype)
    rec = 0
    for j in range(steps):
        up[:, 1:-1] = u
        a, e = up[:, :-2], up[:, 2:]
        transport = (a * a) * (-c) + (e * e) * c
        diffusion = a * d + u * dm + e * d
        u = u + dt32 * (-0.5 * transport + diffusion + fi[:, j // f_time])
        if (j + 1) % record_time == 0:
            rec += 1
            out[:, rec] = u
    assert rec == num_t
    return out


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return ((a - b).norm() / b.norm()).item()


def run_ref(u0, f, **kw):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = ref_solve(u0.clone(), f.clone(), **kw)
    return out, buf.getvalue().strip()


CASES = {
    # name: (N, nx0, Nt_f, keywords of the call); the long case last
    'D1': (2, 100, 15, dict(visc=VISC, T=0.1, num_t=9)),
    'D2': (2, 50, 10, dict(visc=VISC, T=0.1, num_t=10, s=257)),
    'B': (2, 240, 160, dict(visc=VISC, T=0.25, num_t=160)),
    'C': (2, 1920, 40, dict(visc=VISC, T=0.25, num_t=10)),
    'A': (4, 120, 80, dict(visc=VISC, T=8.0, num_t=80, output_space_downsample=False)),
}
FILE_OF = {'A': '', 'D1': '', 'D2': '', 'B': '_b', 'C': '_c'}
ERRORS = {
    # name: (u0 shape, f shape, keywords)
    'E_f_past_end': ((2, 120), (2, 7, 120), dict(visc=VISC, T=0.1, num_t=10)),           # 7 does not divide 7680
    'E_records_past_end': ((2, 120), (2, 10, 120), dict(visc=VISC, T=0.1, num_t=100)),    # 7680 // 76 = 101 records
    'E_f_time_zero': ((2, 120), (2, 10, 120), dict(visc=VISC, T=0.0001, num_t=4)),        # 8 steps < Nt_f
    'E_record_time_zero': ((2, 120), (2, 4, 120), dict(visc=VISC, T=0.0001, num_t=80)),   # 8 steps < num_t
    'E_num_t_zero': ((2, 120), (2, 4, 120), dict(visc=VISC, T=0.0001, num_t=0)),
    'E_sub_s_zero': ((2, 120), (2, 4, 120), dict(visc=VISC, T=0.0001, num_t=4, s=64)),    # s < nx0 with output_space_downsample
    'E_batch_mismatch': ((3, 120), (2, 4, 120), dict(visc=VISC, T=0.0001, num_t=4)),
}


def plan_ints(u0_shape, f_shape, T, num_t, s=1920, dt=DT):
    steps = math.ceil(T / dt)
    return steps, math.floor(steps / num_t), math.floor(steps / f_shape[1]), int(s / u0_shape[-1])


def main():
    torch.set_num_threads(1)          # [N, 1922] rows: per-op overhead dominates, threads only add to it
    files = {'': {}, '_b': {}, '_c': {}}
    manifest = {'signature': {k: (None if p.default is inspect.Parameter.empty else repr(p.default))
                              for k, p in inspect.signature(ref_solve).parameters.items()},
                'cases': {}, 'errors': {}}
    for i, (name, (N, nx0, Nt_f, kw)) in enumerate(CASES.items()):
        torch.manual_seed(1000 + i)
        u0, f = make_data_varying_f(N, N, nx0, Nt_f, 'cpu')
        u0, f = u0.float().contiguous(), f.float().contiguous()
        ref, line = run_ref(u0, f, **kw)
        s = kw.get('s', 1920)
        steps, record_time, f_time, sub_s = plan_ints(u0.shape, f.shape, kw['T'], kw['num_t'], s)
        assert line == f'{steps} {record_time} {f_time}', (name, line)
        full = dict(visc=kw['visc'], T=kw['T'], num_t=kw['num_t'], dt=DT, s=s)
        sub = sub_s if kw.get('output_space_downsample', True) else 1
        f32 = sliced_solve(u0, f, dtype=torch.float32, **full)[:, :, ::sub]
        r32 = rel_l2(f32, ref)
        assert r32 <= 1e-5, (name, r32)
        ex = sliced_solve(u0, f, dtype=torch.float64, **full)[:, :, ::sub]
        print(name, 'ref-vs-slicing(fp32)', r32, 'ref-vs-exact', rel_l2(ref, ex), flush=True)
        g = files[FILE_OF[name]]
        g[f'{name}/u0'], g[f'{name}/f'] = u0.numpy(), f.numpy()
        if name == 'A':           # what eval_ddpm_burgers.py:204 keeps (every 16th column) + the final row J_actual reads, full width
            g['A/ref_cols16'], g['A/exact_d_cols16'] = ref[:, :, ::16].numpy(), (ex[:, :, ::16] - ref[:, :, ::16].double()).float().numpy()
            g['A/ref_last'], g['A/exact_d_last'] = ref[:, -1].numpy(), (ex[:, -1] - ref[:, -1].double()).float().numpy()
        else:
            g[f'{name}/ref'], g[f'{name}/exact_d'] = ref.numpy(), (ex - ref.double()).float().numpy()
        manifest['cases'][name] = dict(file=f'ref_burgers_solver{FILE_OF[name]}.npz', u0_shape=list(u0.shape), f_shape=list(f.shape),
                                       kwargs=kw, out_shape=list(ref.shape), printed=line, steps=steps, record_time=record_time,
                                       f_time=f_time, sub_s=sub_s, ref_vs_slicing_fp32=r32, ref_vs_exact=rel_l2(ref, ex))
    for name, (us, fs, kw) in ERRORS.items():
        torch.manual_seed(7)
        u0, f = torch.randn(*us), torch.randn(*fs)
        buf = io.StringIO()
        try:
            with contextlib.redirect_stdout(buf):
                ref_solve(u0, f, **kw)
            raise SystemExit(f'{name}: the reference did not fail')
        except (ZeroDivisionError, IndexError, ValueError, AssertionError) as e:
            exc = type(e).__name__
        print(name, exc, flush=True)
        manifest['errors'][name] = dict(u0_shape=list(us), f_shape=list(fs), kwargs=kw, exception=exc, printed=buf.getvalue().strip())
    for suffix, g in files.items():
        np.savez_compressed(os.path.join(HERE, f'ref_burgers_solver{suffix}.npz'), **g)
    with open(os.path.join(HERE, 'ref_burgers_solver_manifest.json'), 'w') as fh:
        json.dump(manifest, fh, indent=1)
    for fn in sorted(os.listdir(HERE)):
        if fn.startswith('ref_burgers_solver'):
            print(fn, os.path.getsize(os.path.join(HERE, fn)))


if __name__ == '__main__':
    main()
