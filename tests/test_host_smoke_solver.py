"""Host side of the smoke control-evaluation solver (wdno_amd.smoke_solver and the dataset.evaluate_solver drop-in): no GPU, no library."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import smoke_solver_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, M = R.load_golden()

EXACT_FRAMES = 9          # frames 0..8 of the fp64 restatement: the stored frames 0 and 8 and nine entries of the ratio


def test_geometry_equals_reference_masks():
    """Every mask of the reference's FluidSimulation / get_bucket_mask and the five diagonals of its pressure matrix, exactly."""
    from wdno_amd.smoke_solver import geometry
    g = geometry()
    for key, got in (('fluid', g.fluid), ('active', g.active), ('velocity', g.velocity_mask), ('fluid_ext', g.fluid_ext),
                     ('active_ext', g.active_ext), ('buckets', g.buckets), ('bucket_concat', g.bucket_concat), ('set_zero', g.set_zero)):
        want = G[f'masks/{key}']
        assert got.shape == want.shape and np.array_equal(got, want), key
    assert g._fluid_mask.shape == (1, 127, 127, 1) and g._velocity_mask.shape == (1, 128, 128, 2)
    diag = g.matrix_diagonals()
    for k in (0, 1, -1, 127, -127):
        want = G[f'matrix/diag_{k}']
        assert diag[k].shape == want.shape and np.array_equal(diag[k], want), k


def test_geometry_from_other_rectangles():
    from wdno_amd.smoke_solver import BUCKETS, geometry
    g = geometry(obstacles=[((2, 3), (10, 20))], buckets=BUCKETS)
    assert g.fluid.sum() == 127 * 127 - 6 and not g.fluid[10:12, 20:23].any()
    assert g.velocity_mask[10, 20].tolist() == [0, 0] and g.velocity_mask[12, 20].tolist() == [1, 0] and g.velocity_mask[9, 20].tolist() == [1, 1]
    assert g is not geometry() and geometry() is geometry()


@pytest.mark.parametrize('nt', [32, 64, 128, 256])
@pytest.mark.parametrize('nx', [64, 128])
def test_plan_integers(nt, nx):
    from wdno_amd.smoke_solver import plan
    p = plan((3, nx, nx), (3, nt, nx, nx), (3, nt, nx, nx))
    assert (p['time_interval'], p['space_interval']) == (int(256 / nt), int(128 / nx)) == (256 // nt, 128 // nx)
    assert (p['B'], p['nt'], p['nx'], p['num_t'], p['max_iter'], p['threads']) == (3, nt, nx, 256, 500, 512)
    assert p['accuracy'] == float(np.float32(1e-8))
    assert plan((3, nx, nx), (3, nt, nx, nx), threads=1024)['threads'] == 1024


def test_plan_raises_reference_errors():
    """np.tile(...).reshape(256, 128, 128) of evaluate_solver.py:152-154 fails with ValueError for these shapes."""
    from wdno_amd.smoke_solver import plan
    for d, c1, c2 in (((2, 64, 64), (2, 48, 64, 64), None),            # nt does not divide 256
                      ((2, 48, 48), (2, 32, 48, 48), None),            # nx does not divide 128
                      ((2, 64, 64), (2, 32, 64, 64), (2, 64, 64, 64)),  # c2 of another shape
                      ((2, 32, 32), (2, 32, 64, 64), None)):           # density of another grid
        with pytest.raises(ValueError):
            plan(d, c1, c2)
    with pytest.raises(ValueError):
        plan((2, 64, 64), (2, 32, 64, 64), threads=256)


@pytest.mark.parametrize('name', ['mid', 'off'])
def test_fp64_restatement_reproduces_exact(name):
    """tests/smoke_solver_ref.py in fp64 with the pressure solved to 1e-12 is the fixture's `exact`: the first EXACT_FRAMES frames, compared
    on the stored frames among them (0 and 8, cells ::2) and on the ratio's first EXACT_FRAMES entries; rel-L2 < 1e-9."""
    from wdno_amd.smoke_solver import geometry, init_velocity
    d0, c1, c2 = R.case_inputs(G, M, name)
    out = R.simulate(geometry(), init_velocity(), d0, c1, c2, np.float64, 'exact', frames=EXACT_FRAMES)
    for field in ('density', 'zero_density', 'velocity'):
        _, exact = R.stored(G, name, field, 'sub')
        got = out[field][::8, ::2, ::2]
        err = R.rel_l2(got, exact[:got.shape[0]])
        print(name, field, err)
        assert err < 1e-9, (field, err)
    _, exact = R.stored(G, name, 'smoke_out', None)
    assert np.allclose(out['smoke_out'], exact[:EXACT_FRAMES], rtol=1e-9, atol=1e-300)


def test_fixture_condition():
    shares = {k: c['final_share'] for k, c in M['cases'].items()}
    assert sum(0.01 <= s <= 0.95 for s in shares.values()) >= 2, shares
    assert abs(shares['mid'] - 0.176) < 1e-3 and abs(shares['off'] - 0.0227) < 1e-4


def _run(code):
    return subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd=ROOT)


def test_dropin_imports_without_phiflow():
    """`from dataset.evaluate_solver import *` (inference_2d.py:23) with only this tree on the path: the names the pipeline uses arrive,
    nothing of PhiFlow or matplotlib is loaded, and a plotting helper asked for without the reference behind says so."""
    from wdno_amd import tree_path
    code = ('import sys\n'
            f'sys.path[:0] = [{ROOT!r}, {tree_path("smoke")!r}]\n'
            'from dataset.evaluate_solver import *\n'
            'import dataset.evaluate_solver as m\n'
            'for n in m.__all__:\n'
            '    assert n in globals(), n\n'
            'for n in ("init_sim", "init_velocity_", "solver", "get_bucket_mask", "get_bucket_mask_torch", "gif_density"):\n'
            '    assert n in m.__all__ and callable(globals()[n]), n\n'
            'assert "phi" not in sys.modules and "matplotlib" not in sys.modules and "wdno_amd._lib" not in sys.modules\n'
            'sim = init_sim()\n'
            'assert sim._fluid_mask.shape == (1, 127, 127, 1)\n'
            'v = init_velocity_()\n'
            'assert v.shape == (1, 128, 128, 2) and v.dtype.name == "float32" and float(v[0, 3, 4, 1]) == float(__import__("numpy").float32(0.2)) and not v[..., 0].any()\n'
            'lst, concat, zero = get_bucket_mask()\n'
            'assert len(lst) == 7 and concat.shape == zero.shape == (128, 128) and concat.sum() + zero.sum() == 128 * 128\n'
            'tl, tc, tz = get_bucket_mask_torch("cpu")\n'
            'assert tl[1].shape == (1, 128, 128) and tc.shape == (1, 128, 128) and float(tl[1].sum()) == lst[1].sum()\n'
            'try:\n'
            '    gif_density(None, zero=False)\n'
            'except AttributeError as e:\n'
            '    print("OK", "no reference module" in str(e))\n')
    out = _run(code)
    assert out.returncode == 0 and 'OK True' in out.stdout, out.stderr[-2000:]


def test_forked_child_guard_raises():
    """solver() in a forked child of a process that has initialised the GPU raises a RuntimeError naming evaluate_controls before anything
    touches the device (here the parent only claims an initialised GPU: no GPU is needed, and the library is never loaded)."""
    from wdno_amd import tree_path
    code = ('import os, sys\n'
            f'sys.path[:0] = [{ROOT!r}, {tree_path("smoke")!r}]\n'
            'import numpy as np, torch\n'
            'from dataset.evaluate_solver import *\n'
            'torch.cuda.is_initialized = lambda: True\n'
            'pid = os.fork()\n'
            'if pid == 0:\n'
            '    code = 1\n'
            '    try:\n'
            '        solver(init_sim(), init_velocity_(), np.zeros((64, 64), np.float32), np.zeros((32, 64, 64), np.float32), np.zeros((32, 64, 64), np.float32))\n'
            '    except RuntimeError as e:\n'
            '        code = 0 if "evaluate_controls" in str(e) and "fork" in str(e) and "wdno_amd._lib" not in sys.modules else 2\n'
            '    os._exit(code)\n'
            '_, status = os.waitpid(pid, 0)\n'
            'print("CHILD", os.waitstatus_to_exitcode(status))\n')
    out = _run(code)
    assert out.returncode == 0 and 'CHILD 0' in out.stdout, (out.stdout, out.stderr[-2000:])


def test_plan_and_geometry_need_no_library_or_gpu():
    code = ('import sys\n'
            f'sys.path.insert(0, {ROOT!r})\n'
            'from wdno_amd.smoke_solver import plan, geometry\n'
            'plan((25, 64, 64), (25, 32, 64, 64)); geometry()\n'
            'assert "wdno_amd._lib" not in sys.modules\n'
            'import torch\n'
            'assert not torch.cuda.is_initialized()\n'
            'print("OK")\n')
    out = _run(code)
    assert out.returncode == 0 and 'OK' in out.stdout, out.stderr[-2000:]
