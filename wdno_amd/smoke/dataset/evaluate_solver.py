"""MI355X drop-in for smoke/dataset/evaluate_solver.py: `solver` (l.135-196), the flow re-simulation that scores a designed smoke control
(inference_2d.py:310-380), runs as one HIP launch (wdno_amd.smoke_solver, csrc/smoke_solver.hip). No PhiFlow: `init_sim()` returns the
masks of the reference's domain (wdno_amd.smoke_solver.Geometry), built in numpy.

Same signatures and return values as the reference: init_sim, init_velocity_, solver, get_bucket_mask, get_bucket_mask_torch. The plotting
helpers (gif_density, gif_vel, gif_control, get_bound, ...) come from the reference's module when that is on sys.path behind this tree;
nothing of it (PhiFlow, matplotlib) is loaded until such a name is asked for.

solver() scores ONE simulation per call. The reference driver starts one forked process per sample around it
(InferencePipeline.multi_evaluate_control); a process that has initialised the GPU cannot be forked like that, so solver() raises in such
a child without touching the device. Score a batch with wdno_amd.smoke_solver.evaluate_controls(pred, data): one process, one launch."""
import numpy as np
import torch

import wdno_amd
from wdno_amd import smoke_solver as _solver

__all__ = ['init_sim', 'init_velocity_', 'solver', 'get_bucket_mask', 'get_bucket_mask_torch',
           'gif_density', 'gif_vel', 'gif_control', 'get_bound', 'draw_pic', 'plot_vector_field_128', 'plot_control_field_128']

_reference_getattr = wdno_amd.reference_fallthrough('dataset.evaluate_solver', __file__)


def init_sim():
    """The domain of evaluate_solver.py:60-63 as masks (no FluidSimulation object)."""
    return _solver.geometry()


def init_velocity_():
    """[1, 128, 128, 2] fp32: vx = 0, vy = 0.2 (evaluate_solver.py:74-76)."""
    return _solver.init_velocity(vx=0, vy=0.2)


def solver(sim, init_velocity, init_density, c1, c2, dt=1):
    """init_velocity [128, 128, 2] (or with a leading 1), init_density [nx, nx], c1, c2 [nt, nx, nx], numpy. Returns the reference's
    tuple: densitys, zero_densitys [256, 128, 128] (fp32 values in fp64 arrays), velocitys [256, 128, 128, 2] fp32, c1, c2 tiled to
    [256, 128, 128], smoke_out_record [256, 128, 128] fp64 (the frame's ratio in every cell)."""
    _solver.check_not_forked_gpu_child('dataset.evaluate_solver.solver')
    if dt != 1:
        raise ValueError(f'smoke solver: the kernel advects with dt = 1 (the only value the reference passes), got {dt}')
    d0, c1, c2 = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))[None] for a in (init_density, c1, c2))
    density, zero_density, velocity, ratio = _solver.solve(d0, c1, c2, init_velocity=np.asarray(init_velocity, np.float32), geom=sim)
    record = np.tile(ratio[0].numpy()[:, None, None], (1, _solver.GRID, _solver.GRID))
    tiled = lambda c: _solver.tile_control(c)[0].numpy()
    return (density[0].numpy().astype(np.float64), zero_density[0].numpy().astype(np.float64), velocity[0].numpy(), tiled(c1), tiled(c2),
            record)


def get_bucket_mask():
    """evaluate_solver.py:111-132: (the seven bucket masks, their union, the set-zero mask), [128, 128] float64 each."""
    g = _solver.geometry()
    return [g.buckets[i].copy() for i in range(7)], g.bucket_concat.copy(), g.set_zero.copy()


def get_bucket_mask_torch(device):
    """evaluate_solver.py:199-223: the same as fp32 tensors with a leading 1 on `device`."""
    lst, concat, set_zero = get_bucket_mask()
    t = lambda a: torch.from_numpy(a).to(torch.float32).to(device).unsqueeze(0)
    return [t(m) for m in lst], t(concat), t(set_zero)


def _from_reference(name):
    def call(*args, **kwargs):
        return _reference_getattr(name)(*args, **kwargs)
    call.__name__ = call.__qualname__ = name
    call.__doc__ = f'{name} of the reference\'s dataset/evaluate_solver.py, loaded when first called.'
    return call


for _name in __all__[5:]:       # the plotting helpers: names that `import *` can deliver without loading the reference
    globals()[_name] = _from_reference(_name)


def __getattr__(name):          # anything else of the reference module
    return _reference_getattr(name)
