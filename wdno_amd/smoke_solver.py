"""The smoke control-evaluation solver on MI355X: the flow re-simulation that scores a designed smoke control (`solver()` of
smoke/dataset/evaluate_solver.py:135-196, called once per sample by InferencePipeline.multi_evaluate_control, smoke/inference_2d.py:310-380)
as one launch of csrc/smoke_solver.hip (wdno_smoke_solve): one workgroup per simulation, all 256 frames, each frame's conjugate-gradient
pressure solve included.

geometry()          -- plain numpy: the masks of the reference's domain (127 x 127 cells, the rectangles of
                       build_obstacles_pi_128, the bucket rectangles of get_bucket_mask) from lists of rectangles; a caller may pass others.
                       init_sim()'s DomainBoundary([(True, True), (True, True)]) is an OPEN domain: the fluid mask is padded with ones,
                       the active mask with zeros (pressure 0 outside), so the system is non-singular.
plan()              -- pure Python: the reference's host integers (time_interval, space_interval), the reference's errors for shapes it cannot
                       run, and the kernel configuration (threads per simulation).
solve()             -- launches on torch's current stream. CPU inputs are solved on the current GPU and returned on the CPU.
evaluate_controls() -- the contract of multi_evaluate_control, in one process and one launch.

Per frame the kernel does what the reference does: compose the velocity (interior from the previous frame, 16-cell rim from the control),
mask it, take the divergence, solve the masked 5-point system by CG in fp32 (start x = 0, stop at max|r| < 1e-8 or after 500 iterations,
with the reference's aliased first iteration: its `momentum` and `residual` are one array until the first update), subtract the masked
pressure gradient, advect the two densities and update the seven bucket sums. Accumulations are wider than the reference's: the CG dot
products are summed pairwise (fp32 inside a wave, fp64 across waves), the pressure itself -- the sum of the CG steps a p, where the
reference's fp32 `pressure += a * momentum` loses most of its accuracy -- is summed in fp64 (fp32 registers for 16 steps at a time), and
the advection weights and the bucket sums are fp64 as in the reference. Every field the steps read is fp32; the order is fixed, so a simulation has the same bits alone, at any
position of a batch, in every call and with every configuration.

The 0/0 case. The reference's CG divides by sum(p * A p) without a guard. Its loop tests max|r| >= 1e-8 first, so an exactly divergence-free
frame leaves with zero pressure before the division; the kernel does the same, and it also leaves (keeping the pressure it has) if
sum(p * A p) is exactly zero with a non-zero residual, where the reference would go on with NaN.
"""
import os

import numpy as np
import torch

NUM_T = 256           # frames of one simulation (evaluate_solver.py:149)
GRID = 128            # staggered grid; the cell grid is GRID - 1
MAX_ITER = 500        # SparseCGPressureSolver.solve_with_boundaries: max_iterations
ACCURACY = 1e-8       # get_envolve: accuracy
THREADS = (1024, 512)  # supported workgroup sizes (16 / 32 cells of the padded 128 x 128 pressure grid per thread)
DEFAULT_THREADS = 512  # 3-4 % faster than 1024 at batch 1 and 50, within 0.5 % at 256 (profiles/smoke_solver.md); the bits are the same

# (size (y, x), origin (y, x)) of build_obstacles_pi_128 (evaluate_solver.py:32-58)
OBSTACLES = (
    ((1, 96), (16, 16)),
    ((8, 1), (16, 16)), ((16, 1), (40, 16)), ((40, 1), (72, 16)),
    ((8, 1), (16, 112)), ((16, 1), (40, 112)), ((40, 1), (72, 112)),
    ((1, 8), (112, 16)), ((1, 16), (112, 40)), ((1, 16), (112, 72)), ((1, 8), (112, 104)),
    ((16, 1), (64, 48)), ((16, 1), (96, 48)), ((16, 1), (64, 80)), ((16, 1), (96, 80)),
    ((1, 128 - 40 - 40), (40, 40)),
)
# (y, x, len_y, len_x) of get_bucket_mask (evaluate_solver.py:112-113); the second is the target
BUCKETS = (
    (112, 24 - 2, 127 - 112, 16 + 4), (112, 56 - 2, 127 - 112, 16 + 4), (112, 88 - 2, 127 - 112, 16 + 4),
    (24 - 2, 0, 16 + 4, 16), (56 - 2, 0, 16 + 4, 16), (24 - 2, 112, 16 + 4, 127 - 112), (56 - 2, 112, 16 + 4, 127 - 112),
)


class Geometry:
    """Masks of one domain. fluid / active [n, n] int8 (1 = fluid cell); fluid_ext / active_ext [n + 2, n + 2] (what the pressure
    solver sees: open boundary, fluid padded with ones, active with zeros; closed: both with zeros); velocity_mask [n + 1, n + 1, 2] (component 0 along the last axis); buckets [7, n + 1, n + 1],
    bucket_concat, set_zero [n + 1, n + 1] float64 as in get_bucket_mask. _fluid_mask, _active_mask, _velocity_mask have the shapes of
    the reference's FluidSimulation attributes."""

    def __init__(self, obstacles=OBSTACLES, buckets=BUCKETS, n=GRID - 1, open_boundary=True):
        if n != GRID - 1:
            raise ValueError(f'smoke solver: the kernel is built for {GRID - 1} x {GRID - 1} cells, got {n}')
        if len(buckets) != 7:
            raise ValueError(f'smoke solver: seven buckets expected, got {len(buckets)}')
        self.n = n
        fluid = np.ones((n, n), np.int8)
        for (h, w), (y, x) in obstacles:
            fluid[y:y + h, x:x + w] = 0
        self.fluid, self.active = fluid, fluid.copy()
        self.fluid_ext = np.pad(self.fluid, 1, 'constant', constant_values=1 if open_boundary else 0)      # flow.py:418-423
        self.active_ext = np.pad(self.active, 1, 'constant')
        fe = self.fluid_ext
        along_y = np.minimum(fe[1:, 1:], fe[:-1, 1:])           # face between cells (i - 1, j) and (i, j)
        along_x = np.minimum(fe[1:, 1:], fe[1:, :-1])           # face between cells (i, j - 1) and (i, j)
        self.velocity_mask = np.stack([along_x, along_y], -1)
        m = n + 1
        self.buckets = np.zeros((7, m, m))
        self.bucket_concat = np.zeros((m, m))
        self.set_zero = np.ones((m, m))
        for k, (y, x, ly, lx) in enumerate(buckets):
            self.buckets[k, y:y + ly, x:x + lx] = 1
            self.bucket_concat[y:y + ly, x:x + lx] = 1
            self.set_zero[y:y + ly, x:x + lx] = 0
        self._fluid_mask = self.fluid.reshape(1, n, n, 1)
        self._active_mask = self.active.reshape(1, n, n, 1)
        self._velocity_mask = self.velocity_mask.reshape(1, m, m, 2)

    def stencil(self):
        """The masked 5-point matrix of sparse_pressure_matrix (phi/solver/sparse.py:27-78) as five [n, n] float32 planes:
        centre = min(-(fluid neighbours), -1), and the couplings active[neighbour] * active[self] to (i - 1, j), (i + 1, j), (i, j - 1),
        (i, j + 1)."""
        fe, ae = self.fluid_ext.astype(np.float32), self.active_ext.astype(np.float32)
        c = ae[1:-1, 1:-1]
        centre = np.minimum(-(fe[2:, 1:-1] + fe[:-2, 1:-1] + fe[1:-1, 2:] + fe[1:-1, :-2]), -1)
        return dict(centre=centre, up=ae[:-2, 1:-1] * c, down=ae[2:, 1:-1] * c, left=ae[1:-1, :-2] * c, right=ae[1:-1, 2:] * c)

    def matrix_diagonals(self):
        """The diagonals 0, +1, -1, +n, -n of the [n^2, n^2] matrix (row-major cells), as scipy's A.diagonal(k) gives them."""
        s, n = self.stencil(), self.n
        flat = {k: v.reshape(-1) for k, v in s.items()}
        return {0: flat['centre'], 1: flat['right'][:-1], -1: flat['left'][1:], n: flat['down'][:-n], -n: flat['up'][n:]}

    def device_masks(self, device):
        """The four arrays the kernel reads, fp32 on `device` (cached per device)."""
        cache = self.__dict__.setdefault('_dev', {})
        key = str(device)
        if key not in cache:
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
            cache[key] = (t(self.fluid_ext), t(self.active_ext), t(self.velocity_mask),
                          t(np.concatenate([self.buckets, self.set_zero[None]], 0)))
        return cache[key]


_default_geometry = None


def geometry(obstacles=None, buckets=None):
    """The reference's domain (cached) or, with other rectangle lists, a domain of the caller's."""
    global _default_geometry
    if obstacles is None and buckets is None:
        if _default_geometry is None:
            _default_geometry = Geometry()
        return _default_geometry
    return Geometry(OBSTACLES if obstacles is None else obstacles, BUCKETS if buckets is None else buckets)


def init_velocity(vx=0.0, vy=0.2):
    """init_velocity_() of evaluate_solver.py:66-76: [1, 128, 128, 2] fp32, component 0 = vx, component 1 = vy."""
    v = np.empty((1, GRID, GRID, 2), np.float32)
    v[..., 0], v[..., 1] = vx, vy
    return v


_default_init_velocity = init_velocity          # solve() has a parameter of that name


def plan(density_shape, c_shape, c2_shape=None, threads=None):
    """Host integers of one call and the kernel configuration. density_shape [B, nx, nx], c_shape [B, nt, nx, nx]. Raises what the
    reference raises for shapes it cannot run: its np.tile(...).reshape(256, 128, 128) fails with ValueError when nt does not divide
    256 or nx does not divide 128, and when c2 has another shape than c1 (evaluate_solver.py:150-154)."""
    c2_shape = c_shape if c2_shape is None else c2_shape
    B, nt, nx = int(c_shape[0]), int(c_shape[1]), int(c_shape[2])
    if nt <= 0 or nx <= 0:
        raise ZeroDivisionError(f'smoke solver: empty control {tuple(c_shape)} (the reference divides 256 by nt and 128 by nx)')
    time_interval, space_interval = int(NUM_T / nt), int(GRID / nx)
    if tuple(c_shape[2:]) != (nx, nx) or nx * space_interval != GRID:
        raise ValueError(f'smoke solver: control {tuple(c_shape)} is not [B, nt, nx, nx] with nx dividing {GRID}')
    if nt * time_interval != NUM_T:
        raise ValueError(f'smoke solver: nt = {nt} of control {tuple(c_shape)} does not divide {NUM_T}')
    if tuple(c2_shape) != tuple(c_shape):
        raise ValueError(f'smoke solver: c2 {tuple(c2_shape)} differs from c1 {tuple(c_shape)}')
    if tuple(density_shape) != (B, nx, nx):
        raise ValueError(f'smoke solver: init_density {tuple(density_shape)} is not [{B}, {nx}, {nx}] as the controls {tuple(c_shape)} need')
    threads = DEFAULT_THREADS if threads is None else int(threads)
    if threads not in THREADS:
        raise ValueError(f'smoke solver: {threads} threads per simulation is not a supported configuration: {THREADS}')
    return dict(B=B, nt=nt, nx=nx, time_interval=time_interval, space_interval=space_interval, num_t=NUM_T, max_iter=MAX_ITER,
                accuracy=float(np.float32(ACCURACY)), threads=threads)


# A process that has initialised the GPU must not be forked into workers that use it (the reference driver's one-process-per-sample
# pattern): remember in the parent whether the GPU was up when a fork happened, and in the child that it is one.
_fork_state = {'gpu_before_fork': False, 'forked': False}


def _before_fork():
    _fork_state['gpu_before_fork'] = bool(torch.cuda.is_initialized())


def _after_fork_in_child():
    _fork_state['forked'] = True


os.register_at_fork(before=_before_fork, after_in_child=_after_fork_in_child)


def check_not_forked_gpu_child(what='wdno_amd.smoke_solver.solve'):
    """Raises in a forked child of a process that had initialised the GPU, before anything touches the device."""
    # the hooks above exist only if this module was imported before the fork; torch's own record covers a child that imports it afterwards
    if (_fork_state['forked'] and _fork_state['gpu_before_fork']) or torch.cuda._is_in_bad_fork():
        raise RuntimeError(f'{what} was called in a forked child of a process that has initialised the GPU; a GPU context does not survive '
                           'fork(). Do not start one process per sample: score the whole batch in the parent with '
                           'wdno_amd.smoke_solver.evaluate_controls(pred, data), which is one process and one launch.')


WS_FLOATS = 9 * GRID * GRID          # per simulation: velocity (2 planes), pressure, two densities x two buffers, fp64 pressure sum (2)


def solve(init_density, c1, c2, init_velocity=None, frames=None, geom=None, threads=None):
    """The reference's solver() for a batch: init_density [B, nx, nx], c1, c2 [B, nt, nx, nx]; init_velocity [128, 128, 2] (or with a
    leading 1; default init_velocity_()), shared by the batch. Returns (density, zero_density, velocity, smoke_out): fp32
    [B, F, 128, 128], the same, [B, F, 128, 128, 2], and the fp64 ratio smoke_outs[1] / (sum(smoke_outs) + sum(zero_density)) of every
    frame, [B, 256]. `frames` (a sequence of increasing frame numbers) selects the F frames that are written; None writes all 256.
    The result is on init_density's device and belongs to no autograd graph."""
    check_not_forked_gpu_child()
    from wdno_amd import _lib
    home = init_density.device
    dev = home if init_density.is_cuda else torch.device('cuda', torch.cuda.current_device())
    pl = plan(tuple(init_density.shape), tuple(c1.shape), tuple(c2.shape), threads)
    geom = geometry() if geom is None else geom
    if frames is None:
        frames = range(NUM_T)
    frames = [int(f) for f in frames]
    if any(f < 0 or f >= NUM_T for f in frames) or any(b <= a for a, b in zip(frames, frames[1:])):
        raise ValueError('smoke solver: frames must be increasing frame numbers in [0, 256)')
    slot = np.full(NUM_T, -1, np.int32)
    slot[frames] = np.arange(len(frames), dtype=np.int32)
    B, nf = pl['B'], len(frames)
    lib = _lib.load()
    with torch.no_grad(), torch.cuda.device(dev):
        d0 = init_density.detach().to(dev, torch.float32).contiguous()
        c1c = c1.detach().to(dev, torch.float32).contiguous()
        c2c = c2.detach().to(dev, torch.float32).contiguous()
        v0 = _default_init_velocity() if init_velocity is None else init_velocity
        v0 = torch.as_tensor(np.asarray(v0) if not torch.is_tensor(v0) else v0).detach().to(dev, torch.float32).reshape(GRID, GRID, 2).contiguous()
        fluid, active, vmask, buckets = geom.device_masks(dev)
        slot_d = torch.from_numpy(slot).to(dev)
        density = torch.empty(B, nf, GRID, GRID, device=dev, dtype=torch.float32)
        zero_density = torch.empty_like(density)
        velocity = torch.empty(B, nf, GRID, GRID, 2, device=dev, dtype=torch.float32)
        ratio = torch.empty(B, NUM_T, device=dev, dtype=torch.float64)
        ws = torch.empty(B, WS_FLOATS, device=dev, dtype=torch.float32)
        desc = _lib.SmokeSolveDesc(B=B, nt=pl['nt'], nx=pl['nx'], time_interval=pl['time_interval'], space_interval=pl['space_interval'],
                                   num_t=pl['num_t'], max_iter=pl['max_iter'], n_out=nf, threads=pl['threads'], accuracy=pl['accuracy'])
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.wdno_smoke_solve(d0.data_ptr(), c1c.data_ptr(), c2c.data_ptr(), v0.data_ptr(), fluid.data_ptr(), active.data_ptr(),
                                        vmask.data_ptr(), buckets.data_ptr(), slot_d.data_ptr(), density.data_ptr(),
                                        zero_density.data_ptr(), velocity.data_ptr(), ratio.data_ptr(), ws.data_ptr(), desc, stream),
                   'wdno_smoke_solve')
        out = (density, zero_density, velocity, ratio)
        if home != dev:
            torch.cuda.current_stream(dev).synchronize()
    return out if home == dev else tuple(o.to(home) for o in out)


def tile_control(c, frames=None):
    """The reference's np.tile of a control [B, nt, nx, nx] up to [B, 256 (or the chosen frames), 128, 128]."""
    B, nt, nx = c.shape[0], c.shape[1], c.shape[2]
    ti, si = NUM_T // nt, GRID // nx
    t_idx = torch.arange(NUM_T, device=c.device) // ti
    if frames is not None:
        t_idx = t_idx[torch.as_tensor(list(frames), device=c.device)]
    s_idx = torch.arange(GRID, device=c.device) // si
    return c[:, t_idx][:, :, s_idx][:, :, :, s_idx]


def evaluate_controls(pred, data, geom=None, threads=None):
    """InferencePipeline.multi_evaluate_control (smoke/inference_2d.py:310-380) for the whole batch in one launch. pred, data
    [B, nt, 6, nx, nx] (channels: density, vel_x, vel_y, control_x, control_y, smoke share). As there, the interior of the control is
    zeroed on a copy, pred_[:, :, 3:5, 8:56, 8:56] = 0; the initial density is data[:, 0, 0], the controls pred_[:, :, 3] and pred_[:, :, 4].
    Returns solver_out [B, 256, 6, 128, 128] fp32 on pred's device: density, vel_x, vel_y, control_x, control_y (tiled), smoke share."""
    pred = pred.detach().clone()
    pred[:, :, 3:5, 8:56, 8:56] = 0          # indirect control (inference_2d.py:337)
    c1, c2 = pred[:, :, 3], pred[:, :, 4]
    density, _, velocity, ratio = solve(data[:, 0, 0], c1, c2, geom=geom, threads=threads)
    out = torch.empty(pred.shape[0], NUM_T, 6, GRID, GRID, device=density.device, dtype=torch.float32)
    out[:, :, 0] = density
    out[:, :, 1] = velocity[..., 0]
    out[:, :, 2] = velocity[..., 1]
    out[:, :, 3] = tile_control(c1.detach().to(density.device, torch.float32))
    out[:, :, 4] = tile_control(c2.detach().to(density.device, torch.float32))
    out[:, :, 5] = ratio.to(torch.float32)[:, :, None, None]
    return out
