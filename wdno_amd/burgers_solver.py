"""The Burgers control-evaluation solver on MI355X: burgers_numeric_solve_free (burgers/ddpm_burgers/generate_burgers.py:104-204) as one
launch of csrc/burgers.hip (wdno_burgers_solve).

plan()  -- pure Python: the reference's host integers (steps, record_time, f_time, sub_s), its fp32 constants, the reference's exceptions
           for inputs it cannot run, and the kernel configuration (waves per trajectory W, grid points per lane P).
solve() -- launches on torch's current stream. CPU inputs are solved on the current GPU and returned on the CPU (the reference function is
           device-agnostic and its callers pass whatever they hold).

Configuration rule (W, P): a trajectory is one workgroup of W waves whose lanes hold P contiguous points each (64 W P >= s).
  - N >= 4 x CUs (a wave per SIMD already, throughput-bound): W = 1, the fewest waves, no barrier.
  - otherwise (latency-bound: one workgroup per CU at most): W = the smallest power of two such that N W >= 4 x CUs, capped at 8 (at 16 the
    per-step barrier of 16 waves costs more than the halved points per lane save), and at least the waves s needs.
  P is then the smallest supported value with 64 W P >= s. The evaluation call (N = 25, s = 1920, 256 CUs) takes W = 8, P = 4; a batch of
  1 024 takes W = 1, P = 32.
"""
import math

import numpy as np
import torch

DT = 1 / 76800
WAVES = (1, 2, 4, 8, 16)
POINTS = (2, 4, 8, 16, 32)
MAX_POINTS_AT = {1: 32, 2: 32, 4: 32, 8: 32, 16: 16}        # 16 waves x 32 points would not fit 128 VGPRs a lane
MAX_S = max(64 * w * MAX_POINTS_AT[w] for w in WAVES)     # 16 384
CUS_MI355X = 256


def configs(s):
    """Every supported (W, P) that covers a grid of s points."""
    return [(w, p) for w in WAVES for p in POINTS if p <= MAX_POINTS_AT[w] and 64 * w * p >= s]


def choose_config(N, s, cu_count=CUS_MI355X):
    """The rule of the module docstring."""
    if s > MAX_S:
        raise ValueError(f'burgers solver: s = {s} grid points exceed the largest configuration ({MAX_S})')
    if N >= 4 * cu_count:
        w = 1
    else:
        w = 1
        while w < 8 and N * w < 4 * cu_count:
            w *= 2
    while 64 * w * MAX_POINTS_AT[w] < s:
        w *= 2
    p = next(p for p in POINTS if p <= MAX_POINTS_AT[w] and 64 * w * p >= s)
    return w, p


def plan(u0_shape, f_shape, T, dt=DT, num_t=80, s=120 * 16, output_space_downsample=True, visc=0.01, cu_count=CUS_MI355X, config=None):
    """Host integers, fp32 constants and (W, P) of one call; raises what the reference raises (generate_burgers.py:120-201), in its order."""
    if u0_shape[0] != f_shape[0]:                                      # l.120
        raise AssertionError(f'batch of u0 ({u0_shape[0]}) and f ({f_shape[0]}) differ')
    N, nx0, Nt_f, nxf = int(u0_shape[0]), int(u0_shape[-1]), int(f_shape[1]), int(f_shape[-1])
    sub_s = int(s / nx0)                                               # l.127 (ZeroDivisionError for an empty grid, as there)
    steps = math.ceil(T / dt)                                          # l.138
    record_time = math.floor(steps / num_t)                            # l.146 (ZeroDivisionError for num_t == 0)
    f_time = math.floor(steps / Nt_f)                                  # l.148
    if steps > 0:                                                      # the loop, l.176-195
        if f_time == 0 or record_time == 0:
            raise ZeroDivisionError('integer division or modulo by zero')
        if (steps - 1) // f_time >= Nt_f:
            raise IndexError(f'index {(steps - 1) // f_time} is out of bounds for dimension 1 with size {Nt_f}')
        if steps // record_time > num_t:
            raise IndexError(f'index {num_t} is out of bounds for dimension 2 with size {num_t}')
    if steps >= 2 ** 30:
        raise ValueError(f'burgers solver: {steps} steps do not fit the kernel\'s 32-bit step counters')
    if output_space_downsample and sub_s == 0:                         # l.200: trajectory[:, :, ::0]
        raise ValueError('slice step cannot be zero')
    if not output_space_downsample:
        sub_s = 1
    if config is None:
        config = choose_config(N, s, cu_count)
    elif tuple(config) not in configs(s):
        raise ValueError(f'burgers solver: (W, P) = {tuple(config)} is not a supported configuration for s = {s}: {configs(s)}')
    dx = (1.0 - 0.0) / (s + 1)                                         # l.135
    return dict(N=N, s=s, nx0=nx0, nt_f=Nt_f, nxf=nxf, steps=steps, record_time=record_time, f_time=f_time, num_t=int(num_t),
                sub_s=sub_s, out_cols=-(-s // sub_s), waves=int(config[0]), points=int(config[1]),
                c=float(np.float32(1.0 / (2 * dx))),                   # l.163: [-1, 1] / (2 dx) -> fp32
                d=float(np.float32(visc * 1.0 / dx ** 2)),             # l.165: visc [1, -2, 1] / dx^2 -> fp32
                dm=float(np.float32(visc * -2.0 / dx ** 2)),
                dt=float(np.float32(dt)))


def solve(u0, f, visc, T, num_t=80, dt=DT, s=120 * 16, output_space_downsample=True, config=None):
    """burgers_numeric_solve_free on the GPU: [N, num_t + 1, out_cols] fp32 on u0's device; config forces (W, P)."""
    from wdno_amd import _lib
    home = u0.device
    dev = u0.device if u0.is_cuda else torch.device('cuda', torch.cuda.current_device())
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    pl = plan(tuple(u0.shape), tuple(f.shape), T, dt, num_t, s, output_space_downsample, visc, cus, config)
    lib = _lib.load()
    with torch.no_grad(), torch.cuda.device(dev):
        u0c = u0.detach().to(dev, torch.float32).contiguous()
        fc = f.detach().to(dev, torch.float32).contiguous()
        alloc = torch.empty if pl['steps'] > 0 else torch.zeros           # no steps: the reference's rows 1.. stay zero
        out = alloc(pl['N'], pl['num_t'] + 1, pl['out_cols'], device=dev, dtype=torch.float32)
        desc = _lib.BurgersDesc(**{k: (max(v, 0) if k == 'steps' else v) for k, v in pl.items()})
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.wdno_burgers_solve(u0c.data_ptr(), fc.data_ptr(), out.data_ptr(), desc, stream), 'wdno_burgers_solve')
    return out if home == dev else out.to(home)
