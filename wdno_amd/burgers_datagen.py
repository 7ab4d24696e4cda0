"""The Burgers data-set generator on MI355X: make_data_varying_f + burgers_numeric_solve_free + the two slices of
generate_data_burgers_equation (burgers/ddpm_burgers/generate_burgers.py:207-368) as one launch of csrc/burgers_datagen.hip
(wdno_burgers_generate) per batch.

The reference's forcing is separable,

    f[n, t, x] = sum_{k<8} (amp_k[n] X_k[n, x]) T_k[n, t],   X_k = exp(-0.5 (x - loc)^2 / sig^2),   T_k = 2 exp(-0.5 (ts - loc')^2 / sig'^2),

and multiplying in the reference's order (amp * exp_space * exp_time) and summing the terms in order gives its dense f [N, t, s] bit for
bit. So the kernel takes two small tables per trajectory, AX [8, s] = amp_k X_k and TT [t, 8] = T_k (102 KB at the data-set shape, against
9.8 MB of dense f), and forms each control interval's forcing in registers. The dense tensor, 7.9 GB per batch of 800 and several times
that in `.repeat` temporaries, never exists.

draw()          -- the tables and u0 from torch's global generator in make_data_varying_f's call order: after torch.manual_seed(S) on a
                   device it draws what the reference draws there, batch after batch.
dense_forcing() -- the [N, t, s] tensor in torch, for tests and for comparing with the dense path only.
plan()          -- pure Python: the solver's host integers (burgers_solver.plan), the slice strides st, sx, the record shapes, the
                   reference's errors, and the kernel configuration (W, P).
generate()      -- one launch on torch's current stream: (u_rec, f_rec) = (trajectory[:, :, ::sx], f[:, ::st, ::sx]) on the GPU.
write_dataset() -- generate_data_burgers_equation + main: batches, the shuffle, the train / test files data_burgers_1d.py and
                   wave_trans.py read. The reference's log.yaml step is omitted.

Configuration rule (W, P): burgers_solver.choose_config. A batch of 800 at s = 1920 takes (2, 16); in the sweep of
profiles/burgers_datagen.md (4, 8) was 2 % faster in one run, not enough to give this module a rule of its own.

    python -m wdno_amd.burgers_datagen --train_samples 24000 --test_samples 6000 --end_time 8 --nt 80 --nx 120 --save_path data/1d/
"""
import argparse
import os
import random

import numpy as np
import torch

from wdno_amd import burgers_solver as _solver
from wdno_amd.burgers_solver import CUS_MI355X, DT

TERMS = 8            # rand_f terms summed into f: one with a dense amplitude, seven with a randint(2) mask (generate_burgers.py:266-269)
S_FINE, T_FINE = 120 * 16, 80 * 16          # the grid generate_data_burgers_equation simulates on (l.327-328)
VISC = 0.01


def draw(N, s=S_FINE, t=T_FINE, device='cuda', amp_compensate=2):
    """u0 [N, s], AX [N, 8, s], TT [N, t, 8] (fp32 on `device`) of make_data_varying_f(N, N, s, t, device, amp_compensate): the same
    calls on torch's global generator in the same order, the same expressions without the `.repeat`s."""
    xmin = 0.0; xmax = 1.0
    delta_x = (xmax - xmin) / (s + 1)
    x = torch.linspace(xmin + delta_x, xmax - delta_x, s).to(device)
    tmin = 0.0; tmax = 1.0
    delta_t = (tmax - tmin) / (t + 1)
    ts = torch.linspace(tmin + delta_t, tmax - delta_t, t).to(device)

    loc1 = torch.rand(N, 1, device=device) * 0.2 + 0.2
    amp1 = torch.rand(N, 1, device=device) * 2
    sig1 = torch.rand(N, 1, device=device) * 0.1 + 0.05
    gauss1 = amp1 * torch.exp(-0.5 * (x.view(1, -1) - loc1) ** 2 / sig1 ** 2)
    loc2 = torch.rand(N, 1, device=device) * 0.2 + 0.6
    amp2 = torch.rand(N, 1, device=device) * 2 - 2
    sig2 = torch.rand(N, 1, device=device) * 0.1 + 0.05
    gauss2 = amp2 * torch.exp(-0.5 * (x.view(1, -1) - loc2) ** 2 / sig2 ** 2)
    u0 = gauss1 + gauss2

    ax, tt = [], []
    for k in range(TERMS):
        if k:
            amp = torch.randint(2, (N, 1, 1), device=device).float() * \
                (torch.rand(N, 1, 1, device=device) * 3 - 1.5)
        else:
            amp = (torch.rand(N, 1, 1, device=device) * 3 - 1.5)
        loc = torch.rand(N, 1, 1, device=device)
        sig = torch.rand(N, 1, 1, device=device) * 0.3 + 0.1
        exp_space = torch.exp(-0.5 * (x.view(1, 1, -1) - loc) ** 2 / sig ** 2)                       # [N, 1, s]
        loc = torch.rand(N, 1, 1, device=device)
        sig = torch.rand(N, 1, 1, device=device) * 0.3 + 0.1
        exp_time = amp_compensate * torch.exp(-0.5 * (ts.view(1, -1, 1) - loc) ** 2 / sig ** 2)      # [N, t, 1]
        ax.append(amp * exp_space)
        tt.append(exp_time)
    return u0, torch.cat(ax, dim=1).to(torch.float32).contiguous(), torch.cat(tt, dim=2).to(torch.float32).contiguous()


def dense_forcing(AX, TT, alpha=1.):
    """make_data_varying_f's f [N, t, s] from the tables, in torch: (amp X_k) T_k summed over k in order, then the clamp of l.272-273."""
    f = AX[:, 0, None, :] * TT[:, :, 0, None]
    for k in range(1, AX.shape[1]):
        f += AX[:, k, None, :] * TT[:, :, k, None]
    f = f.to(torch.float32)
    if alpha != 1.:
        f = (f * alpha).clamp(-10., 10.)
    return f


def choose_config(N, s, cu_count=CUS_MI355X):
    """(W, P) of the table kernel: the solver's rule (profiles/burgers_datagen.md has the sweep at N = 800)."""
    return _solver.choose_config(N, s, cu_count)


def plan(N, s, t, T, num_t, nx, nt, dt=DT, visc=VISC, cu_count=CUS_MI355X, config=None):
    """Host integers of one generate() call on N trajectories of s points under t control intervals: the solver's plan for u0 [N, s] and
    f [N, t, s] (steps, record_time, f_time, the fp32 constants, (W, P)) plus st = int(t / nt), sx = int(s / nx) and the record shapes.
    Raises what the reference raises, in its order: the solver's ZeroDivisionError / IndexError (generate_burgers.py:335), then
    ZeroDivisionError for nt or nx of 0 and ValueError for a zero slice step, nt > t or nx > s (l.346-347)."""
    N, s, t = int(N), int(s), int(t)
    if config is None and s <= _solver.MAX_S:
        config = choose_config(N, s, cu_count)
    pl = _solver.plan((N, s), (N, t, s), T, dt=dt, num_t=num_t, s=s, output_space_downsample=True, visc=visc, cu_count=cu_count,
                      config=config)
    st, sx = int(t / nt), int(s / nx)
    if st == 0 or sx == 0:
        raise ValueError('slice step cannot be zero')
    pl.update(t=t, st=st, sx=sx, f_rows=-(-t // st), cols=-(-s // sx))
    pl.update(u_shape=(N, pl['num_t'] + 1, pl['cols']), f_shape=(N, pl['f_rows'], pl['cols']))
    return pl


def generate(u0, AX, TT, T, num_t, nx, nt, alpha=1., visc=VISC, dt=DT, config=None):
    """One batch of the data set in one launch on the current stream: u_rec [N, num_t + 1, ceil(s / sx)] = the reference's
    trajectory[:, :, ::sx] and f_rec [N, ceil(t / st), ceil(s / sx)] = its f[:, ::st, ::sx], fp32 on the GPU, for u0 [N, s], AX [N, 8, s],
    TT [N, t, 8] of draw(). No [N, t, s] tensor is formed. config forces (W, P)."""
    from wdno_amd import _lib
    if u0.dim() != 2 or AX.dim() != 3 or TT.dim() != 3 or AX.shape[1] != TERMS or TT.shape[2] != TERMS:
        raise ValueError(f'burgers datagen: u0 [N, s], AX [N, {TERMS}, s], TT [N, t, {TERMS}] expected, got {tuple(u0.shape)}, '
                         f'{tuple(AX.shape)}, {tuple(TT.shape)}')
    N, s, t = int(u0.shape[0]), int(u0.shape[1]), int(TT.shape[1])
    if AX.shape[0] != N or TT.shape[0] != N or AX.shape[2] != s:
        raise ValueError(f'burgers datagen: u0 {tuple(u0.shape)}, AX {tuple(AX.shape)} and TT {tuple(TT.shape)} do not belong together')
    dev = u0.device if u0.is_cuda else torch.device('cuda', torch.cuda.current_device())
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    pl = plan(N, s, t, T, num_t, nx, nt, dt, visc, cus, config)
    lib = _lib.load()
    with torch.no_grad(), torch.cuda.device(dev):
        u0c, axc, ttc = (v.detach().to(dev, torch.float32).contiguous() for v in (u0, AX, TT))
        alloc = torch.empty if pl['steps'] > 0 else torch.zeros           # no steps: the reference's rows 1.. stay zero
        u_rec = alloc(pl['u_shape'], device=dev, dtype=torch.float32)
        f_rec = torch.empty(pl['f_shape'], device=dev, dtype=torch.float32)
        desc = _lib.BurgersGenerateDesc(N=N, s=s, t=t, steps=max(pl['steps'], 0), record_time=pl['record_time'], f_time=pl['f_time'],
                                        num_t=pl['num_t'], st=pl['st'], sx=pl['sx'], f_rows=pl['f_rows'], cols=pl['cols'],
                                        waves=pl['waves'], points=pl['points'], clamp=int(alpha != 1.), c=pl['c'], d=pl['d'], dm=pl['dm'],
                                        dt=pl['dt'], alpha=float(alpha))
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.wdno_burgers_generate(u0c.data_ptr(), axc.data_ptr(), ttc.data_ptr(), u_rec.data_ptr(), f_rec.data_ptr(), desc, stream),
                   'wdno_burgers_generate')
    return u_rec, f_rec


def shuffle_split(n, train_samples):
    """The reference's shuffle (generate_burgers.py:355-365) on Python's global `random`: (train indices, test indices)."""
    shuffled_indices = random.sample(range(n), n)
    return shuffled_indices[:train_samples], shuffled_indices[train_samples:]


def check_files(save_path):
    """The reference's guard with the names the files are actually written to (save_path + 'train', string concatenation)."""
    if os.path.exists(save_path + 'train') or os.path.exists(save_path + 'test'):
        raise FileExistsError('File already exists. Remove both train and test sets before generating new ones.')


def write_dataset(save_path, train_samples, test_samples, batch_size=800, end_time=8., start_time=0., nt=80, nx=120, alpha=1., seed=0,
                  s=S_FINE, t=T_FINE, device=None):
    """generate_data_burgers_equation + main of the reference's script (uniform = False, varying_f = True): seeds torch, numpy and
    `random` with `seed`, draws and solves int((train + test) / batch_size) batches on the s x t grid (one launch each), shuffles with
    random.sample and saves {'f': [n, nt, nx], 'u': [n, nt + 1, nx]} (fp32, CPU) with torch.save to save_path + 'train' and
    save_path + 'test' (string concatenation, as there). FileExistsError if either exists. The reference's log.yaml is not written.
    Returns (train count, test count)."""
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)
    check_files(save_path)
    os.makedirs(save_path, exist_ok=True)          # the reference's check_directory
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    f_list, trajectory_list = [], []
    for _ in range(int((test_samples + train_samples) / batch_size)):
        u0, AX, TT = draw(batch_size, s, t, device)
        u_rec, f_rec = generate(u0, AX, TT, end_time - start_time, nt, nx, nt, alpha=alpha, visc=VISC, dt=DT)
        f_list.append(f_rec.cpu())
        trajectory_list.append(u_rec.cpu())
    f = torch.cat(f_list)
    trajectory = torch.cat(trajectory_list)
    train, test = shuffle_split(trajectory.shape[0], train_samples)
    torch.save({'f': f[train].float(), 'u': trajectory[train].float()}, save_path + 'train')
    torch.save({'f': f[test].float(), 'u': trajectory[test].float()}, save_path + 'test')
    print('Data saved')
    return len(train), len(test)


def parser():
    """The reference script's arguments, names and defaults (generate_burgers.py:409-450)."""
    ap = argparse.ArgumentParser(description='Generating PDE data')
    ap.add_argument('--experiment', type=str, default='burgers', help='unused')
    ap.add_argument('--device', type=str, default='cuda:0', help='Used device')
    ap.add_argument('--num_f', default=1000, type=int, help='unused')
    ap.add_argument('--num_u0', default=100, type=int, help='unused')
    ap.add_argument('--train_samples', type=int, default=90000, help='Samples in the training dataset')
    ap.add_argument('--test_samples', type=int, default=10000, help='Samples in the test dataset')
    ap.add_argument('--log', type=eval, default=False, help='unused')
    ap.add_argument('--uniform_u_f', default=False, type=eval, help='True is not implemented, as in the reference')
    ap.add_argument('--varying_f', type=eval, default=True, help='If the force sample varies over time')
    ap.add_argument('--nt', type=int, default=10, help='Time grids (f has nt values over time and u is stamped nt + 1 times, including u0)')
    ap.add_argument('--nx', type=int, default=128, help='Space grids.')
    ap.add_argument('--start_time', type=float, default=0., help='Physical starting time')
    ap.add_argument('--end_time', type=float, default=1., help='Physical ending time')
    ap.add_argument('--alpha', type=float, default=1., help='How much w is shifted from the original dataset')
    ap.add_argument('--save_path', type=str, default='data/1d/', help='Which path to save the result into')
    ap.add_argument('--seed', type=int, default=0, help='Random seed')
    return ap


def main(argv=None):
    """The reference script's command line. --device names the torch device to generate on and is used as given; the reference instead sets
    CUDA_VISIBLE_DEVICES to the string's last character. --num_f, --num_u0, --log and --experiment are accepted and ignored."""
    args = parser().parse_args(argv)
    if args.uniform_u_f:
        raise NotImplementedError('Not using the setting of Nf * Nu0 = Nsamples for now.')
    assert args.varying_f, 'Only supports varying_f when every f is paired with a different u0'
    n = write_dataset(args.save_path, args.train_samples, args.test_samples, end_time=args.end_time, start_time=args.start_time, nt=args.nt,
                      nx=args.nx, alpha=args.alpha, seed=args.seed, device=args.device)
    print(f'{n[0]} train and {n[1]} test trajectories written to {args.save_path}train, {args.save_path}test')


if __name__ == '__main__':
    main()
