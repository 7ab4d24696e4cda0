"""Plain-numpy restatement of the smoke control-evaluation solver (smoke/dataset/evaluate_solver.py:135-196 with the PhiFlow pieces it
calls: phi/flow.py:294-333, phi/math/nd.py:332-427,603-614, phi/solver/base.py:56-103, phi/solver/sparse.py:27-78), written with slices.
Test infrastructure only.

simulate(..., dtype=np.float32, cg='reference') follows the reference step by step in fp32: the CG with its aliased first iteration, the
stop at max|r| < 1e-8 or 500 iterations, scipy's fp64 interpolation of the fp32 density. simulate(..., dtype=np.float64, cg='exact') is
the arbiter's exact value: the same chain on the same fp32 inputs in fp64, with the pressure system solved to max|r| <= 1e-12 by fp64 CG
(started at 0, so the iterate stays in the range of the singular Neumann matrix)."""
import numpy as np

NUM_T, G, N = 256, 128, 127


def apply_A(st, p):
    """The masked 5-point matrix on a [127, 127] field; st = Geometry.stencil() in p's dtype."""
    out = np.zeros_like(p)                               # scipy's csc product adds a row's terms by ascending column
    out[1:, :] += st['up'][1:, :] * p[:-1, :]
    out[:, 1:] += st['left'][:, 1:] * p[:, :-1]
    out += st['centre'] * p
    out[:, :-1] += st['right'][:, :-1] * p[:, 1:]
    out[:-1, :] += st['down'][:-1, :] * p[1:, :]
    return out


def cg_reference(st, k, accuracy=1e-8, max_iterations=500):
    """conjugate_gradient (phi/solver/base.py:56-103) as it runs: x = 0, momentum and residual are the SAME array until the first
    `momentum = residual + b * momentum`, and residual is updated in place."""
    dt = k.dtype.type
    x = np.zeros_like(k)
    residual = k.copy()
    momentum = residual                                  # the alias
    Ap = apply_A(st, momentum)
    it = 0
    while np.max(np.abs(residual)) >= dt(accuracy):
        if it == max_iterations:
            break
        tmp = np.sum(momentum * Ap)
        a = np.sum(momentum * residual) / tmp
        x += a * momentum
        residual -= a * Ap                              # first pass: momentum changes with it
        b = -np.sum(residual * Ap) / tmp
        momentum = residual + b * momentum
        Ap = apply_A(st, momentum)
        it += 1
    return x, it, float(np.max(np.abs(residual)))


def cg_exact(st, k, tol=1e-12, max_iterations=20000):
    """Textbook fp64 CG from x = 0 to max|r| <= tol."""
    x = np.zeros_like(k)
    r = k.copy()
    p = r.copy()
    rr = np.sum(r * r)
    it = 0
    while np.max(np.abs(r)) > tol and it < max_iterations:
        Ap = apply_A(st, p)
        a = rr / np.sum(p * Ap)
        x += a * p
        r -= a * Ap
        rr_new = np.sum(r * r)
        p = r + (rr_new / rr) * p
        rr = rr_new
        it += 1
    return x, it, float(np.max(np.abs(r)))


def divergence(v):
    return (v[1:, :-1, 1] - v[:-1, :-1, 1]) + (v[:-1, 1:, 0] - v[:-1, :-1, 0])


def gradient(p):
    pp = np.pad(p, 1, 'symmetric')
    g = np.empty((G, G, 2), p.dtype)
    g[..., 1] = pp[1:, 1:] - pp[:-1, 1:]
    g[..., 0] = pp[1:, 1:] - pp[1:, :-1]
    return g


def advect(field, v, dt=1):
    """_advect_centered_field + the scipy backend's resample: coordinates idx - v dt in the velocity's dtype, clamped to [0, 127],
    linear interpolation in fp64 with 0 outside [0, 126], rounded to the field's dtype."""
    ci = (v[1:, :-1, 1] + v[:-1, :-1, 1]) / 2
    cj = (v[:-1, 1:, 0] + v[:-1, :-1, 0]) / 2
    ii, jj = np.meshgrid(np.arange(N), np.arange(N), indexing='ij')
    yi = np.maximum(0, np.minimum(N, ii.astype(v.dtype) - ci * dt)).astype(np.float64)
    xj = np.maximum(0, np.minimum(N, jj.astype(v.dtype) - cj * dt)).astype(np.float64)
    inside = (yi <= N - 1) & (xj <= N - 1)
    yi, xj = np.minimum(yi, N - 1), np.minimum(xj, N - 1)
    i0 = np.minimum(np.floor(yi).astype(np.int64), N - 2)
    j0 = np.minimum(np.floor(xj).astype(np.int64), N - 2)
    wy, wx = yi - i0, xj - j0
    f = field.astype(np.float64)
    val = ((1 - wy) * (1 - wx) * f[i0, j0] + (1 - wy) * wx * f[i0, j0 + 1] + wy * (1 - wx) * f[i0 + 1, j0] + wy * wx * f[i0 + 1, j0 + 1])
    return np.where(inside, val, 0.0).astype(field.dtype)


def tile_inputs(init_density, c1, c2):
    nt, nx = c1.shape[0], c1.shape[1]
    ti, si = int(NUM_T / nt), int(G / nx)
    d = np.repeat(np.repeat(init_density, si, 0), si, 1)
    up = lambda c: np.repeat(np.repeat(np.repeat(c, ti, 0), si, 1), si, 2)
    return d, up(c1), up(c2)


def simulate(geom, init_velocity, init_density, c1, c2, dtype=np.float32, cg='reference', frames=NUM_T, dt=1):
    """Returns dict(density [F, 128, 128], zero_density, velocity [F, 128, 128, 2] in `dtype`, smoke_out [F] fp64, the CG's iterations [F] and final max|r| (of its recursive residual) [F])
    for the first `frames` frames. Inputs are taken as fp32 values (the pipeline's dtype)."""
    st = {k: v.astype(dtype) for k, v in geom.stencil().items()}
    vmask = geom.velocity_mask.astype(dtype)
    d0, C1, C2 = tile_inputs(np.asarray(init_density, np.float32), np.asarray(c1, np.float32), np.asarray(c2, np.float32))
    dens = d0[:-1, :-1].astype(dtype)
    zdens = dens.copy()
    vel = np.asarray(init_velocity, np.float32).reshape(G, G, 2).astype(dtype)
    outs = np.zeros(7)
    solve = cg_reference if cg == 'reference' else cg_exact
    rec = dict(density=[], zero_density=[], velocity=[], smoke_out=[], iterations=[], residual=[])
    for frame in range(frames):
        cur = np.zeros((G, G, 2), dtype)
        cur[..., 0], cur[..., 1] = C1[frame], C2[frame]
        cur[16:112, 16:112] = vel[16:112, 16:112]
        cur = cur * vmask
        p, it, res = solve(st, divergence(cur))
        vel = (cur - gradient(p) * vmask) * vmask
        dens, zdens = advect(dens, vel, dt), advect(zdens, vel, dt)
        arr = np.zeros((G, G))
        arr[:-1, :-1] = dens
        if np.sum(arr * geom.bucket_concat) > 0:
            for i in range(7):
                outs[i] += np.sum(arr * geom.buckets[i])
            zdens = (zdens * geom.set_zero[:-1, :-1]).astype(dtype)
        zarr = np.zeros((G, G))
        zarr[:-1, :-1] = zdens
        rec['density'].append(arr.astype(dtype)); rec['zero_density'].append(zarr.astype(dtype)); rec['velocity'].append(vel.copy())
        rec['smoke_out'].append(outs[1] / (np.sum(outs) + np.sum(zarr)))
        rec['iterations'].append(it)
        rec['residual'].append(res)
    return {k: np.stack(v) for k, v in rec.items()}


# ---------------------------------------------------------------------------------------------- the reference fixtures
def load_golden():
    """(arrays, manifest) of tests/golden/ref_smoke_solver*.npz (make_ref_smoke_solver_golden.py)."""
    import json
    import os
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
    with open(os.path.join(golden, 'ref_smoke_solver_manifest.json')) as f:
        manifest = json.load(f)
    arrays = {}
    for fn in manifest['files']:
        with np.load(os.path.join(golden, fn)) as z:
            arrays.update(unshuffled(k, z[k]) for k in z.files)
    return arrays, manifest


def shuffled(key, v):
    """(key, array) as stored: arrays of 2-, 4- or 8-byte items go as their byte planes, uint8 [itemsize, ...], under 'key|dtype' (the
    exponent bytes of neighbouring values are alike: zlib gets ~10 % more out of planes than out of interleaved bytes). Lossless."""
    if np.asarray(v).dtype.itemsize < 2 or np.asarray(v).size < 1000:
        return key, v
    v = np.ascontiguousarray(v)
    planes = np.moveaxis(v.view(np.uint8).reshape(v.shape + (v.dtype.itemsize,)), -1, 0)
    return f'{key}|{v.dtype.str}', np.ascontiguousarray(planes)


def unshuffled(key, v):
    if '|' not in key:
        return key, v
    key, dt = key.split('|')
    return key, np.ascontiguousarray(np.moveaxis(v, 0, -1)).view(dt)[..., 0]


def case_inputs(arrays, manifest, name):
    """init_density [nx, nx], c1, c2 [nt, nx, nx] fp32 of a case: the controls are stored as their 16-cell rim (the interior is zero)."""
    nt, nx = manifest['cases'][name]['nt'], manifest['cases'][name]['nx']
    w = 16 * nx // G
    m = np.ones((nx, nx), bool)
    m[w:nx - w, w:nx - w] = False
    out = [arrays[f'{name}/init_density'].astype(np.float32)]
    for key in ('c1_rim', 'c2_rim'):
        c = np.zeros((nt, nx, nx), np.float32)
        c[:, m] = arrays[f'{name}/{key}']
        out.append(c)
    return out


def encode_exact(ref, exact, head=0, scale=None):
    """How the fixtures hold `exact` beside the reference's fp32 `ref`: d = exact - ref as float16 of d / scale with scale = max|d| (the
    exact value to ~5e-4 of the difference, i.e. ~1e-9 of the value, at a quarter of the bytes of fp64), and the first `head` frames of d
    in fp32 as well (the frames the host test recomputes and compares to 1e-9). Returns {suffix: array}."""
    d = np.asarray(exact, np.float64) - np.asarray(ref, np.float64)
    scale = (float(np.max(np.abs(d))) or 1.0) if scale is None else float(scale)
    out = {'_exact_d16': (d / scale).astype(np.float16), '_exact_scale': np.float64(scale)}
    if head:
        out['_exact_d_head'] = d[:head].astype(np.float32)
    return out


def xor_bits(a, b):
    """fp32 arrays as the XOR of their bit patterns: zero wherever they agree (the set-zero density is stored against the density)."""
    return np.ascontiguousarray(a, np.float32).view(np.uint32) ^ np.ascontiguousarray(b, np.float32).view(np.uint32)


def stored(arrays, name, field, which):
    """(reference, exact) of a case's field ('density', 'zero_density', 'velocity', 'smoke_out'); which = 'sub' (frames ::8, cells ::2)
    or 'last'. exact = reference + d in fp64 (encode_exact); the velocity's components are stacked last."""
    if field == 'smoke_out':
        ref = arrays[f'{name}/smoke_out'].astype(np.float64)
        return ref, ref + arrays[f'{name}/smoke_out_exact_d']
    if field.startswith('velocity') and f'{name}/velocity_from' in arrays:      # the same controls as another case: the same velocity
        name = str(arrays[f'{name}/velocity_from'])
    if field == 'velocity':
        rx, ex = stored(arrays, name, 'velocity_x', which)
        ry, ey = stored(arrays, name, 'velocity_y', which)
        return np.stack([rx, ry], -1), np.stack([ex, ey], -1)
    key = f'{name}/{field}_{which}'
    if field == 'zero_density':
        ref = (arrays[key + '_xor_density'] ^ arrays[f'{name}/density_{which}'].view(np.uint32)).view(np.float32).astype(np.float64)
    else:
        ref = arrays[key].astype(np.float64)
    if field == 'zero_density':         # on the density's scale, as the XOR with the density's float16 bits
        d16 = (arrays[key + '_exact_d16_xor_density'] ^ arrays[f'{name}/density_{which}_exact_d16'].view(np.uint16)).view(np.float16)
        d = d16.astype(np.float64) * float(arrays[f'{name}/density_{which}_exact_scale'])
    else:
        d = arrays[key + '_exact_d16'].astype(np.float64) * float(arrays[key + '_exact_scale'])
    if key + '_exact_d_head' in arrays:
        head = arrays[key + '_exact_d_head']
        d[:head.shape[0]] = head
    elif key + '_exact_d_head_xor_density' in arrays:
        head = (arrays[key + '_exact_d_head_xor_density'] ^ arrays[f'{name}/density_{which}_exact_d_head'].view(np.uint32)).view(np.float32)
        d[:head.shape[0]] = head
    return ref, ref + d


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))
