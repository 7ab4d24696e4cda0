"""MI355X drop-in for burgers/ddpm_burgers/generate_burgers.py: `burgers_numeric_solve_free` (l.104-204), the solver that scores a designed
control (eval_ddpm_burgers.py:203, test_util.py:75,77), runs as one HIP launch (wdno_amd.burgers_solver, csrc/burgers.hip).

Same signature and defaults as the reference; `mode` is unused there and here. Every other name (make_data_varying_f,
generate_data_burgers_equation, Diff_mat_1D, VISC, ...) comes from the reference's module when that is on sys.path behind this tree.

Run as a script it is the data-set generator with the reference script's arguments: wdno_amd.burgers_datagen, one HIP launch per batch of
800 trajectories (csrc/burgers_datagen.hip), writing the train / test files data_burgers_1d.py and wave_trans.py read."""
import wdno_amd
from wdno_amd import burgers_solver as _solver

_reference_getattr = wdno_amd.reference_fallthrough('ddpm_burgers.generate_burgers', __file__)


def burgers_numeric_solve_free(u0, f, visc, T, num_t=80, dt=1/76800, s=120*16, mode=None, output_space_downsample=True):
    """Trajectories u [N, num_t + 1, s] (every sub_s-th column with output_space_downsample) of u0 [N, nx0] under the controls
    f [N, Nt_f, nxf]; fp32 on u0's device, not part of any autograd graph."""
    return _solver.solve(u0, f, visc, T, num_t=num_t, dt=dt, s=s, output_space_downsample=output_space_downsample)


def __getattr__(name):          # make_data_varying_f, generate_data_burgers_equation, Diff_mat_1D, VISC, ... from the reference module
    return _reference_getattr(name)


if __name__ == '__main__':
    from wdno_amd import burgers_datagen as _datagen
    _datagen.main()
