"""The smoke control-evaluation solver on the GPU (csrc/smoke_solver.hip through wdno_amd.smoke_solver): the reference fixtures under the
arbiter gate, batch / call / configuration invariance to the bit, frame selection, evaluate_controls, CPU inputs, the divergence-free
frame and a batch beyond one wave of workgroups.

Gate (tests/arbiter.py, the project's standing factor and slack): hip_vs_exact <= 1.5 * ref_vs_exact + 1e-6, rel-L2 against the fp64
chain of the fixture; ref_vs_exact comes from the fixture alone. Each solve is one launch of 256 frames x up to 500 CG iterations."""
import numpy as np
import pytest
import torch

from tests import smoke_solver_ref as R
from tests.arbiter import gate

pytestmark = pytest.mark.gpu

G, M = R.load_golden()
CASES = sorted(M['cases'])
DEV = 'cuda:0'


def _inputs(names):
    d0, c1, c2 = zip(*(R.case_inputs(G, M, n) for n in names))
    return tuple(torch.from_numpy(np.stack(a)).to(DEV) for a in (d0, c1, c2))


_cache = {}


def _solved(name):
    """The full run of one fixture case alone (batch 1, default configuration), computed once."""
    if name not in _cache:
        from wdno_amd.smoke_solver import solve
        _cache[name] = solve(*_inputs([name]))
        torch.cuda.synchronize()
    return _cache[name]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('name', CASES)
def test_reference_cases_under_arbiter_gate(name):
    density, zero_density, velocity, ratio = (t[0].cpu().numpy() for t in _solved(name))
    assert density.shape == (256, 128, 128) and velocity.shape == (256, 128, 128, 2) and ratio.shape == (256,) and ratio.dtype == np.float64
    failed = []
    for field, full in (('density', density), ('zero_density', zero_density), ('velocity', velocity)):
        for which, got in (('sub', full[::8, ::2, ::2]), ('last', full[-1])):
            ref, exact = R.stored(G, name, field, which)
            hip_vs_exact, ref_vs_exact = R.rel_l2(got, exact), R.rel_l2(ref, exact)
            print(f'{name} {field}_{which}: hip_vs_exact {hip_vs_exact:.3e} ref_vs_exact {ref_vs_exact:.3e} hip_vs_ref {R.rel_l2(got, ref):.3e}')
            if not gate(hip_vs_exact, ref_vs_exact):
                failed.append((field, which, hip_vs_exact, ref_vs_exact))
    if M['cases'][name]['counts_for_share']:
        ref, exact = R.stored(G, name, 'smoke_out', None)
        hip_vs_exact, ref_vs_exact = R.rel_l2(ratio, exact), R.rel_l2(ref, exact)
        print(f'{name} smoke_out: hip_vs_exact {hip_vs_exact:.3e} ref_vs_exact {ref_vs_exact:.3e} final share hip {ratio[-1]:.6f} ref {ref[-1]:.6f}')
        if not gate(hip_vs_exact, ref_vs_exact):
            failed.append(('smoke_out', '', hip_vs_exact, ref_vs_exact))
    assert not failed, failed


def test_share_gate_has_cases_that_count():
    assert sum(bool(M['cases'][n]['counts_for_share']) and 0.01 <= M['cases'][n]['final_share'] <= 0.95 for n in CASES) >= 2


def test_batch_call_and_configuration_invariance():
    """Simulation i alone == simulation i of a batch (all cases of the shape plus copies); two calls give the same bits; both workgroup
    sizes give the same bits."""
    from wdno_amd.smoke_solver import THREADS, solve
    names = [n for n in CASES if (M['cases'][n]['nt'], M['cases'][n]['nx']) == (32, 64)]
    assert {'mid', 'off'} <= set(names)
    order = names + names[::-1] + names[:1]
    batch = solve(*_inputs(order))
    for pos, n in enumerate(order):
        assert _same([t[pos] for t in batch], [t[0] for t in _solved(n)]), (pos, n)
    assert _same(solve(*_inputs(['mid'])), _solved('mid'))
    assert set(THREADS) == {1024, 512}
    for threads in THREADS:
        assert _same(solve(*_inputs(['mid']), threads=threads), _solved('mid')), threads


def test_frames_selects_frames_of_the_full_run():
    from wdno_amd.smoke_solver import solve
    frames = [0, 7, 8, 64, 255]
    density, zero_density, velocity, ratio = solve(*_inputs(['off']), frames=frames)
    full = _solved('off')
    assert density.shape == (1, 5, 128, 128) and velocity.shape == (1, 5, 128, 128, 2) and ratio.shape == (1, 256)
    assert torch.equal(density, full[0][:, frames]) and torch.equal(zero_density, full[1][:, frames])
    assert torch.equal(velocity, full[2][:, frames]) and torch.equal(ratio, full[3])
    with pytest.raises(ValueError):
        solve(*_inputs(['off']), frames=[3, 3])


def test_evaluate_controls_equals_solve():
    from wdno_amd.smoke_solver import evaluate_controls, solve, tile_control
    d0, c1, c2 = _inputs(['mid', 'off'])
    gen = torch.Generator().manual_seed(5)
    pred = torch.randn(2, 32, 6, 64, 64, generator=gen).to(DEV)
    pred[:, :, 3], pred[:, :, 4] = c1, c2
    pred[:, :, 3:5, 8:56, 8:56] = torch.randn(2, 32, 2, 48, 48, generator=gen).to(DEV)      # evaluate_controls must zero this itself
    data = torch.randn(2, 256, 1, 64, 64, generator=gen).to(DEV)
    data[:, 0, 0] = d0
    keep = pred.clone()
    out = evaluate_controls(pred, data)
    assert torch.equal(pred, keep)                                                         # the caller's tensor is left alone, as in the reference
    assert out.shape == (2, 256, 6, 128, 128) and out.dtype == torch.float32
    density, _, velocity, ratio = solve(d0, c1, c2)
    assert torch.equal(out[:, :, 0], density) and torch.equal(out[:, :, 1], velocity[..., 0]) and torch.equal(out[:, :, 2], velocity[..., 1])
    assert torch.equal(out[:, :, 3], tile_control(c1)) and torch.equal(out[:, :, 4], tile_control(c2))
    assert torch.equal(out[:, :, 5], ratio.float()[:, :, None, None].expand(-1, -1, 128, 128))
    assert torch.equal(density[0], _solved('mid')[0][0])


def test_dropin_solver_returns_the_reference_tuple():
    """dataset.evaluate_solver.solver(sim, init_velocity, init_density, c1, c2): the reference's 6-tuple with its containers, equal to the
    batched solve."""
    import importlib.util
    import os
    from wdno_amd import tree_path
    spec = importlib.util.spec_from_file_location('_dropin_evaluate_solver', os.path.join(tree_path('smoke'), 'dataset', 'evaluate_solver.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    d0, c1, c2 = R.case_inputs(G, M, 'mid')
    v0 = mod.init_velocity_()
    assert v0.shape == (1, 128, 128, 2)
    out = mod.solver(mod.init_sim(), v0, d0, c1, c2)
    full = [t[0].cpu().numpy() for t in _solved('mid')]
    assert len(out) == 6
    densitys, zero_densitys, velocitys, t1, t2, record = out
    assert densitys.dtype == zero_densitys.dtype == record.dtype == np.float64 and velocitys.dtype == np.float32
    assert densitys.shape == zero_densitys.shape == t1.shape == t2.shape == record.shape == (256, 128, 128) and velocitys.shape == (256, 128, 128, 2)
    assert np.array_equal(densitys, full[0]) and np.array_equal(zero_densitys, full[1]) and np.array_equal(velocitys, full[2])
    assert np.array_equal(record, np.broadcast_to(full[3][:, None, None], (256, 128, 128)))
    assert np.array_equal(t1, np.repeat(np.repeat(np.repeat(c1, 8, 0), 2, 1), 2, 2)) and np.array_equal(t2[255, ::2, ::2], c2[31])


def test_cpu_inputs_come_back_on_the_cpu():
    from wdno_amd.smoke_solver import solve
    out = solve(*(t.cpu() for t in _inputs(['mid'])), frames=[255])
    assert all(t.device.type == 'cpu' for t in out)
    full = _solved('mid')
    assert torch.equal(out[0], full[0][:, 255:].cpu()) and torch.equal(out[3], full[3].cpu())


def test_divergence_free_input_keeps_zero_pressure():
    """Zero velocity and zero controls: the masked divergence is exactly zero in every frame, where the reference's CG would compute 0 / 0
    if it entered its loop. The solve leaves with zero pressure: finite outputs, zero velocity, the density unchanged in every frame."""
    from wdno_amd.smoke_solver import solve
    d0 = _inputs(['mid'])[0]
    zeros = torch.zeros(1, 32, 64, 64, device=DEV)
    density, zero_density, velocity, ratio = solve(d0, zeros, zeros, init_velocity=np.zeros((128, 128, 2), np.float32), frames=[0, 100, 255])
    tiled = d0[0].repeat_interleave(2, 0).repeat_interleave(2, 1).clone()
    tiled[127, :], tiled[:, 127] = 0, 0
    assert all(bool(torch.isfinite(t).all()) for t in (density, zero_density, velocity, ratio))
    assert not velocity.any()
    for k in range(3):
        assert torch.equal(density[0, k], tiled) and torch.equal(zero_density[0, k], tiled)
    assert not ratio.any()


def test_more_simulations_than_compute_units():
    """256 + 1 simulations: more workgroups than one wave of them. Positions 0, 128 and 256 hold the bits of the single-simulation runs."""
    from wdno_amd.smoke_solver import solve
    d0, c1, c2 = _inputs(['mid', 'off'])
    idx = torch.arange(257, device=DEV) % 2
    idx[128] = 1
    density, zero_density, velocity, ratio = solve(d0[idx], c1[idx], c2[idx], frames=[255])
    torch.cuda.synchronize()
    for pos in (0, 128, 256):
        full = _solved(('mid', 'off')[int(idx[pos])])
        assert torch.equal(density[pos, 0], full[0][0, 255]) and torch.equal(zero_density[pos, 0], full[1][0, 255]), pos
        assert torch.equal(velocity[pos, 0], full[2][0, 255]) and torch.equal(ratio[pos], full[3][0]), pos
