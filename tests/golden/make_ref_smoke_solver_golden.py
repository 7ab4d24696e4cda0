"""Golden vectors for the smoke control-evaluation solver, solver() of smoke/dataset/evaluate_solver.py:135-196, by running the
reference and its vendored PhiFlow, unedited.

Build-container only (needs the reference tree):   python tests/golden/make_ref_smoke_solver_golden.py
Writes tests/golden/ref_smoke_solver.npz, ref_smoke_solver_<i>.npz (each under 1 MiB; the manifest lists them) and
ref_smoke_solver_manifest.json -- data only: the reference's masks and matrix diagonals,
each case's inputs (the controls' 16-cell rim only: the interior is zero), the reference's outputs (frames ::8 at cells ::2, the last
frame in full, the full [256] ratio; a case with the controls of an earlier one shares its velocity: `<case>/velocity_from`), `exact - reference` for the same selections (float16 with a
per-array scale, tests/smoke_solver_ref.py: encode_exact; the set-zero density as the XOR of its bits with the density's), the CG iteration count of every frame and
the wall time of the reference call.

PhiFlow 1.x under today's numpy / Python: nothing of it is edited or copied. IPython and imageio are stubbed; collections.Iterable and
the np.bool / np.int / np.float / np.object / np.complex aliases are restored; a meta-path finder compiles every module of the `phi`
package from its source with one syntax-tree rewrite: every non-constant subscript goes through a helper that turns a *list* holding a
slice, None or Ellipsis into a tuple (numpy no longer accepts such lists as indices).

`exact` is the fp64 restatement of tests/smoke_solver_ref.py on the same fp32 inputs, its pressure systems solved to max|r| <= 1e-12 (asserted for every frame; the
worst residual is in the manifest).
Before anything is written the restatement run in fp32 is checked against the reference's fp32 output, which pins it to the reference's
operators."""
import ast
import collections
import collections.abc
import importlib.abc
import importlib.machinery
import importlib.util
import io
import json
import os
import sys
import time
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_SMOKE = os.path.join(os.environ.get('WDNO_REFERENCE', '/root/reference'), 'smoke')
sys.path.insert(0, ROOT)


def _fix_index(idx):
    if isinstance(idx, list) and any(isinstance(e, slice) or e is None or e is Ellipsis for e in idx):
        return tuple(idx)
    return idx


class _WrapSubscripts(ast.NodeTransformer):
    def visit_Subscript(self, node):
        self.generic_visit(node)
        if not isinstance(node.slice, (ast.Constant, ast.Slice)):
            node.slice = ast.Call(func=ast.Name(id='__fix_index__', ctx=ast.Load()), args=[node.slice], keywords=[])
        return node


class _PhiLoader(importlib.machinery.SourceFileLoader):
    def get_code(self, fullname):                       # always from source: never the cached bytecode of the unpatched tree
        path = self.get_filename(fullname)
        tree = _WrapSubscripts().visit(ast.parse(self.get_data(path), path))
        return compile(ast.fix_missing_locations(tree), path, 'exec', dont_inherit=True)

    def exec_module(self, module):
        module.__dict__['__fix_index__'] = _fix_index
        super().exec_module(module)


class _PhiFinder(importlib.abc.MetaPathFinder):
    def find_spec(self, fullname, path=None, target=None):
        if fullname != 'phi' and not fullname.startswith('phi.'):
            return None
        base = os.path.join(REF_SMOKE, *fullname.split('.'))
        if os.path.isdir(base):
            file, pkg = os.path.join(base, '__init__.py'), True
        else:
            file, pkg = base + '.py', False
        if not os.path.isfile(file):
            return None
        return importlib.util.spec_from_file_location(fullname, file, loader=_PhiLoader(fullname, file),
                                                      submodule_search_locations=[base] if pkg else None)


def install():
    for name in ('Iterable', 'Mapping', 'MutableMapping', 'Sequence', 'Callable'):
        if not hasattr(collections, name):
            setattr(collections, name, getattr(collections.abc, name))
    for name, typ in (('bool', bool), ('int', int), ('float', float), ('object', object), ('complex', complex)):
        if name not in np.__dict__:
            setattr(np, name, typ)
    ipy = types.ModuleType('IPython')
    ipy.embed = lambda *a, **k: None
    sys.modules.setdefault('IPython', ipy)
    sys.modules.setdefault('imageio', types.ModuleType('imageio'))
    sys.meta_path.insert(0, _PhiFinder())
    sys.path.insert(1, os.path.join(REF_SMOKE, 'dataset'))
    sys.path.insert(1, REF_SMOKE)


HEAD = 2          # stored frames 0 and 8 carry exact - reference in fp32 too (tests/test_host_smoke_solver.py recomputes frames 0..8)
HEAD_CASES = ('mid', 'off')          # ... of the cases that test runs


def rim_control(rng, nt, nx, amplitude):
    """Standard normal on an 8 x 8 grid, x amplitude, repeated up to nx x nx, interior zeroed (the rim is 16 cells of the 128 grid)."""
    c = rng.standard_normal((nt, 8, 8)).astype(np.float32) * np.float32(amplitude)
    c = np.repeat(np.repeat(c, nx // 8, 1), nx // 8, 2)
    w = 16 * nx // 128
    c[:, w:nx - w, w:nx - w] = 0
    return np.ascontiguousarray(c)


def blob(nx, ys, xs):
    d = np.zeros((nx, nx), np.float32)
    d[ys[0]:ys[1], xs[0]:xs[1]] = 1
    return d


def cases():
    out = {}
    rng = np.random.default_rng(1)
    c1, c2 = rim_control(rng, 32, 64, 0.3), rim_control(rng, 32, 64, 0.3)
    out['mid'] = dict(init_density=blob(64, (40, 48), (28, 36)), c1=c1, c2=c2)
    out['off'] = dict(init_density=blob(64, (40, 48), (36, 46)), c1=c1, c2=c2)
    rng = np.random.default_rng(2)
    out['nt64'] = dict(init_density=blob(64, (40, 48), (26, 34)), c1=rim_control(rng, 64, 64, 0.3), c2=rim_control(rng, 64, 64, 0.3))
    rng = np.random.default_rng(3)
    out['nx128'] = dict(init_density=blob(128, (80, 96), (58, 74)), c1=rim_control(rng, 32, 128, 0.3), c2=rim_control(rng, 32, 128, 0.3))
    return out


def savez9(file, arrays):
    """np.savez_compressed at zlib level 9 (np.load reads it as any .npz)."""
    with zipfile.ZipFile(file, 'w', zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for k, v in arrays.items():
            with zf.open(k + '.npy', 'w', force_zip64=True) as fh:
                np.lib.format.write_array(fh, np.asanyarray(v), allow_pickle=False)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def rim_only(c):
    """[nt, nx, nx] -> the rim cells, flattened per frame (the interior is zero by construction)."""
    nx = c.shape[-1]
    w = 16 * nx // 128
    m = np.ones((nx, nx), bool)
    m[w:nx - w, w:nx - w] = False
    assert not c[:, ~m].any()
    return c[:, m]


def main():
    install()
    import evaluate_solver as E
    from phi.solver import sparse as S
    from tests import smoke_solver_ref as R
    from wdno_amd import smoke_solver as W

    counts = []
    orig_cg = S.conjugate_gradient

    def counting_cg(*a, **k):
        x, it = orig_cg(*a, **k)
        counts.append(int(it))
        return x, it
    S.conjugate_gradient = counting_cg

    sim = E.init_sim()
    geom = W.geometry()
    g = {}
    g['masks/fluid'], g['masks/active'] = sim._fluid_mask[0, :, :, 0], sim._active_mask[0, :, :, 0]
    g['masks/velocity'] = sim._velocity_mask.staggered[0]
    g['masks/fluid_ext'] = sim.extended_fluid_mask[0, :, :, 0]
    g['masks/active_ext'] = sim.extended_active_mask[0, :, :, 0]
    lst, concat, set_zero = E.get_bucket_mask()
    g['masks/buckets'], g['masks/bucket_concat'], g['masks/set_zero'] = np.stack(lst).astype(np.int8), concat.astype(np.int8), set_zero.astype(np.int8)
    A = S.sparse_pressure_matrix([127, 127], sim.extended_active_mask, sim.extended_fluid_mask)
    for k in (0, 1, -1, 127, -127):
        g[f'matrix/diag_{k}'] = np.asarray(A.diagonal(k), np.float32)
    manifest = {'cases': {}, 'selection': 'frames ::8 at cells ::2 (sub), the last frame in full (last), the full [256] ratio',
                'cpu': 'reference wall time in seconds, one process'}
    done = {}
    for name, c in cases().items():
        counts.clear()
        v0 = E.init_velocity_()
        t0 = time.time()
        dens, zdens, vel, _, _, rec = E.solver(sim, v0, c['init_density'].copy(), c['c1'].copy(), c['c2'].copy())
        wall = time.time() - t0
        ratio = rec[:, 0, 0]
        iters = np.array(counts, np.int32)
        assert len(iters) == 256
        f32 = R.simulate(geom, v0, c['init_density'], c['c1'], c['c2'], np.float32, 'reference')
        pins = {k: rel_l2(f32[k], r) for k, r in (('density', dens), ('zero_density', zdens), ('velocity', vel))}
        pins['smoke_out'] = float(np.max(np.abs(f32['smoke_out'] - ratio)))
        print(name, 'wall', round(wall, 1), 'share', ratio[-1], 'iters', iters.min(), iters.mean(), 'restatement(fp32) vs reference', pins, flush=True)
        assert max(pins.values()) <= 1e-3, pins
        ex = R.simulate(geom, v0, c['init_density'], c['c1'], c['c2'], np.float64, 'exact')
        assert ex['residual'].max() <= 1e-12, (name, ex['residual'].max(), ex['iterations'].max())      # every frame's pressure system converged
        rve = {}
        fields = (('density', dens, ex['density']), ('zero_density', zdens, ex['zero_density']),
                  ('velocity_x', vel[..., 0], ex['velocity'][..., 0]), ('velocity_y', vel[..., 1], ex['velocity'][..., 1]))
        twin = next((o for o, oc in done.items() if all(np.array_equal(oc[k], c[k]) for k in ('c1', 'c2'))), None)
        if twin is not None:          # the density never feeds back: the same controls give the same velocity, stored once
            assert np.array_equal(vel, done[twin]['vel'])
            g[f'{name}/velocity_from'] = np.array(twin)
            for key in ('velocity_x', 'velocity_y'):
                rve[key + '_sub'], rve[key + '_last'] = (manifest['cases'][twin]['ref_vs_exact'][key + w] for w in ('_sub', '_last'))
            fields = fields[:2]
        done[name] = dict(c1=c['c1'], c2=c['c2'], vel=vel)
        for key, ref, e in fields:
            for which, r_, e_, head in (('sub', ref[::8, ::2, ::2], e[::8, ::2, ::2], HEAD), ('last', ref[-1], e[-1], 0)):
                r_ = r_.astype(np.float32)
                if key == 'zero_density':          # equal to the density until smoke reaches a bucket: stored as the XOR of the bit patterns
                    g[f'{name}/{key}_{which}_xor_density'] = R.xor_bits(r_, g[f'{name}/density_{which}'])
                else:
                    g[f'{name}/{key}_{which}'] = r_
                head = head if name in HEAD_CASES else 0
                if key == 'zero_density':          # the difference too: on the density's scale, XOR of the float16 bits
                    enc = R.encode_exact(r_, e_, head, scale=g[f'{name}/density_{which}_exact_scale'])
                    g[f'{name}/{key}_{which}_exact_d16_xor_density'] = enc.pop('_exact_d16').view(np.uint16) ^ g[f'{name}/density_{which}_exact_d16'].view(np.uint16)
                    enc.pop('_exact_scale')
                    if head:
                        enc['_exact_d_head_xor_density'] = R.xor_bits(enc.pop('_exact_d_head'), g[f'{name}/density_{which}_exact_d_head'])
                else:
                    enc = R.encode_exact(r_, e_, head)
                for suffix, arr in enc.items():
                    g[f'{name}/{key}_{which}{suffix}'] = arr
                rve[f'{key}_{which}'] = rel_l2(r_, e_)
        g[f'{name}/smoke_out'] = ratio.astype(np.float64)
        g[f'{name}/smoke_out_exact_d'] = (ex['smoke_out'] - ratio).astype(np.float64)
        rve['smoke_out'] = rel_l2(ratio, ex['smoke_out']) if np.linalg.norm(ex['smoke_out']) > 0 else None
        g[f'{name}/init_density'] = c['init_density']
        g[f'{name}/c1_rim'], g[f'{name}/c2_rim'] = rim_only(c['c1']), rim_only(c['c2'])
        g[f'{name}/cg_iterations'] = iters
        print(name, 'reference vs exact', rve, 'exact CG iterations (mean)', float(ex['iterations'].mean()), flush=True)
        manifest['cases'][name] = dict(nt=int(c['c1'].shape[0]), nx=int(c['c1'].shape[1]), final_share=float(ratio[-1]),
                                       counts_for_share=bool(ratio[-1] >= 1e-6), reference_wall_s=wall, cg_iterations_mean=float(iters.mean()),
                                       cg_iterations_min=int(iters.min()), cg_iterations_max=int(iters.max()),
                                       restatement_fp32_vs_reference=pins, ref_vs_exact=rve,
                                       exact_max_residual=float(ex['residual'].max()), exact_cg_iterations_max=int(ex['iterations'].max()))
    assert sum(0.01 <= m['final_share'] <= 0.95 for m in manifest['cases'].values()) >= 2
    # no committed file above 1 MiB: the arrays go, in order, into as many .npz files as that takes; the manifest lists them
    for fn in os.listdir(HERE):
        if fn.startswith('ref_smoke_solver') and fn.endswith('.npz'):
            os.remove(os.path.join(HERE, fn))
    files, cur, cur_size = [], {}, 0
    for k, v in g.items():
        k, v = R.shuffled(k, v)
        buf = io.BytesIO()
        savez9(buf, {k: v})
        size = buf.getbuffer().nbytes
        assert size < 1000000, (k, size)
        if cur and cur_size + size > 1000000:
            files.append(cur)
            cur, cur_size = {}, 0
        cur[k] = v
        cur_size += size
    files.append(cur)
    manifest['files'] = ['ref_smoke_solver.npz'] + [f'ref_smoke_solver_{i}.npz' for i in range(1, len(files))]
    for fn, part in zip(manifest['files'], files):
        savez9(os.path.join(HERE, fn), part)
    with open(os.path.join(HERE, 'ref_smoke_solver_manifest.json'), 'w') as fh:
        json.dump(manifest, fh, indent=1)
    total = 0
    for fn in manifest['files'] + ['ref_smoke_solver_manifest.json']:
        total += os.path.getsize(os.path.join(HERE, fn))
        print(fn, os.path.getsize(os.path.join(HERE, fn)))
    print('total', total)


if __name__ == '__main__':
    main()
