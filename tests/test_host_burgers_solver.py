"""Host side of the Burgers control-evaluation solver (wdno_amd.burgers_solver, the burgers_numeric_solve_free drop-in): no GPU, no library."""
import inspect
import json
import os
import subprocess
import sys

import pytest

from tests.helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _manifest():
    with open(os.path.join(GOLDEN, 'ref_burgers_solver_manifest.json')) as f:
        return json.load(f)


M = _manifest()


def _plan_args(u0_shape, f_shape, kw):
    from wdno_amd.burgers_solver import DT
    return dict(u0_shape=tuple(u0_shape), f_shape=tuple(f_shape), T=kw['T'], dt=kw.get('dt', DT), num_t=kw.get('num_t', 80),
                s=kw.get('s', 1920), output_space_downsample=kw.get('output_space_downsample', True), visc=kw['visc'])


@pytest.mark.parametrize('name', sorted(M['cases']))
def test_plan_reproduces_reference_integers(name):
    """steps / record_time / f_time as the reference printed them (generate_burgers.py:175), sub_s and the output shape."""
    from wdno_amd.burgers_solver import plan
    c = M['cases'][name]
    p = plan(**_plan_args(c['u0_shape'], c['f_shape'], c['kwargs']))
    assert f"{p['steps']} {p['record_time']} {p['f_time']}" == c['printed']
    assert [p['N'], p['num_t'] + 1, p['out_cols']] == c['out_shape']
    assert 64 * p['waves'] * p['points'] >= p['s']


@pytest.mark.parametrize('name', sorted(M['errors']))
def test_plan_raises_reference_exceptions(name):
    from wdno_amd.burgers_solver import plan
    e = M['errors'][name]
    with pytest.raises(Exception) as info:
        plan(**_plan_args(e['u0_shape'], e['f_shape'], e['kwargs']))
    assert type(info.value).__name__ == e['exception']


def test_plan_constants_and_configuration_rule():
    """fp32 constants of generate_burgers.py:163-165 at the default grid; (W, P) by batch size; the widest grid; forced configurations."""
    from wdno_amd import burgers_solver as B
    p = B.plan((25, 120), (25, 80, 120), 8.0, num_t=80, output_space_downsample=False)
    assert p['c'] == 960.5 and p['dm'] == -2 * p['d'] and p['steps'] == 614400
    assert abs(p['d'] * p['dt'] - 0.4805) < 1e-4                          # visc dt / dx^2, under the explicit-Euler limit 0.5
    assert (p['waves'], p['points']) == (8, 4)                            # evaluation batch: latency-bound, many waves
    assert B.choose_config(1024, 1920, 256) == (1, 32)                    # >= 4 x CUs: one wave per trajectory
    assert B.choose_config(4, 16384, 256) in B.configs(16384)
    for N in (1, 25, 100, 800, 1024, 5000):
        for s in (64, 257, 1920, 4096, 16384):
            w, pts = B.choose_config(N, s, 256)
            assert (w, pts) in B.configs(s)
    with pytest.raises(ValueError):
        B.choose_config(4, B.MAX_S + 1)
    with pytest.raises(ValueError):
        B.plan((2, 120), (2, 10, 120), 0.05, num_t=10, config=(1, 4))    # 256 points do not cover 1920
    assert B.plan((2, 120), (2, 10, 120), 0.05, num_t=10, config=(16, 2))['waves'] == 16


def test_plan_needs_no_library_or_gpu():
    code = ('import sys\n'
            f'sys.path.insert(0, {ROOT!r})\n'
            'from wdno_amd.burgers_solver import plan\n'
            'plan((25, 120), (25, 80, 120), 8.0)\n'
            'assert "wdno_amd._lib" not in sys.modules\n'
            'import torch\n'
            'assert not torch.cuda.is_initialized()\n'
            'print("OK")\n')
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and 'OK' in out.stdout, out.stderr[-2000:]


def test_dropin_signature_matches_reference():
    import importlib.util
    spec = importlib.util.spec_from_file_location('_dropin_generate_burgers',
                                                  os.path.join(ROOT, 'wdno_amd', 'burgers', 'ddpm_burgers', 'generate_burgers.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sig = inspect.signature(mod.burgers_numeric_solve_free)
    got = {k: (None if p.default is inspect.Parameter.empty else repr(p.default)) for k, p in sig.parameters.items()}
    assert list(got) == list(M['signature']) and got == M['signature']


def test_dropin_resolution_with_reference_behind(tmp_path):
    """With the burgers tree ahead of a (stand-in) reference tree, eval_ddpm_burgers.py:10's import gets the HIP solver and every other name
    of the module comes from the reference's file."""
    from wdno_amd import tree_path
    fakeb = tmp_path / 'ref_burgers'
    (fakeb / 'ddpm_burgers').mkdir(parents=True)
    (fakeb / 'ddpm_burgers' / '__init__.py').write_text('')
    (fakeb / 'ddpm_burgers' / 'generate_burgers.py').write_text(
        'VISC = 0.01\n'
        'def burgers_numeric_solve_free(*a, **k):\n    return "must not win"\n'
        'def make_data_varying_f(*a, **k):\n    return "reference make_data_varying_f"\n')
    code = (
        'import sys\n'
        f'sys.path[:0] = [{tree_path("burgers")!r}, {str(fakeb)!r}]\n'
        'from ddpm_burgers.generate_burgers import burgers_numeric_solve_free, make_data_varying_f, VISC\n'
        'import ddpm_burgers.generate_burgers as m\n'
        'assert burgers_numeric_solve_free.__module__ == "ddpm_burgers.generate_burgers" and "wdno_amd" in m.__file__\n'
        'assert burgers_numeric_solve_free.__globals__["_solver"].__name__ == "wdno_amd.burgers_solver"\n'
        'assert make_data_varying_f() == "reference make_data_varying_f" and VISC == 0.01\n'
        'try:\n'
        '    m.DoesNotExist\n'
        'except AttributeError as e:\n'
        '    print("OK", type(e).__name__)\n')
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and 'OK AttributeError' in out.stdout, out.stderr[-2000:]
