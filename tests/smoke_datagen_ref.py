"""Plain-numpy restatement of the smoke data-set generator (smoke/dataset/a_gen_train.py:256-327, 363-456, 502-696 and its a_gen_test_64 /
a_gen_test_128 twins) on the operators of tests/smoke_solver_ref.py, the replay of the reference's np.random draws from a seed, and the
seeded noise source of csrc/smoke_datagen.hip (Philox4x32-10 + Box-Muller) in numpy. Test infrastructure only.

generate(..., dtype=np.float32, cg='reference') follows the reference step by step in fp32. generate(..., dtype=np.float64, cg='exact')
is the arbiter's exact value: the same chain in fp64 with the pressure systems solved to max|r| <= 1e-12. Its inputs are the scene and
the noise as the reference uses them: on a kick frame the drawn field rounded to fp32 (the reference stores it in an fp32 array before
anything is computed from it), on an ordinary frame the float64 draw itself, added to the fp64 velocity without the reference's rounding
of the sum to fp32 -- that rounding is part of the reference's (and the kernel's) fp32 evaluation, not of the chain."""
import json
import os

import numpy as np

from tests import smoke_solver_ref as R

G, N = R.G, R.N
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


# ---------------------------------------------------------------------------------------------- the reference's draws, replayed
def replay_scene(rs, scenelength=256):
    """exp2_target_128() then get_per_vel() on the RandomState `rs`, in the reference's call order: six randint (only the taken branch of
    target1_x / target2_x draws), uniform(2, 5), eight scalar normal. Returns dict(xs, ys, vxs, vys, intervals)."""
    m = 5
    start_x = rs.randint(16 + 1 + m, 112 - 10 - m)
    start_y = rs.randint(16 + 1 + m, 40 - 10 - m)
    a = 0 if start_x < 64 - 10 else 1
    t1 = rs.randint(16 + m, 64 - 10) if a == 0 else rs.randint(64, 112 - 10 - m)
    t2 = rs.randint(16 + m, 64 - 10) if a == 0 else rs.randint(64, 112 - 10 - m)
    t3 = rs.randint(50, 80 - 1 - 10)
    end_x = rs.randint(64 - 8, 64 + 8 - 10)
    xs = [int(start_x), int(t1), int(t2), int(t3), int(end_x)]
    ys = [int(start_y), 40, 50, 64, 112]
    dist = [((xs[k + 1] - xs[k]) ** 2 + (ys[k + 1] - ys[k]) ** 2) ** 0.5 for k in range(4)]
    distance = dist[0] + dist[1] + dist[2] + dist[3]
    v = distance / float(scenelength)
    vx = [v * (xs[k + 1] - xs[k]) / dist[k] for k in range(4)]
    vy = [v * (ys[k + 1] - ys[k]) / dist[k] for k in range(4)]
    scale = rs.uniform(2, 5)
    real = lambda vel: rs.normal(vel, abs(vel / 4))
    vxs = [real(scale * c) for c in vx]
    vys = [real(5 * c) for c in vy]
    intervals = [int(scenelength * dist[k] / distance) for k in range(3)]
    return dict(xs=xs, ys=ys, vxs=[float(c) for c in vxs], vys=[float(c) for c in vys], intervals=intervals)


def kick_frames(intervals):
    i0, i1, i2 = (int(i) for i in intervals)
    return [0, i0, i0 + i1, i0 + i1 + i2]


def replay_noise(rs, scene, scenelength):
    """The per-frame draws that follow the scene's on the same RandomState: float64 [scenelength + 1, 128, 128, 2]. A kick frame holds
    the two drawn fields normal(v, |v / 10|, (1, 128, 128)); any other frame normal(0, 0.1, (1, 128, 128, 2))."""
    K = kick_frames(scene['intervals'])
    out = np.empty((scenelength + 1, G, G, 2))
    for f in range(scenelength + 1):
        if f in K:
            k = K.index(f)
            vx, vy = scene['vxs'][k], scene['vys'][k]
            out[f, :, :, 0] = rs.normal(loc=vx, scale=abs(vx / 10), size=(1, G, G))[0]
            out[f, :, :, 1] = rs.normal(loc=vy, scale=abs(vy / 10), size=(1, G, G))[0]
        else:
            out[f] = rs.normal(loc=0, scale=0.1, size=(1, G, G, 2))[0]
    return out


def replay(seed, scenelength):
    """(scene, noise) of np.random.seed(seed) followed by the reference's scene set-up and loop."""
    rs = np.random.RandomState(seed)
    scene = replay_scene(rs, scenelength)
    return scene, replay_noise(rs, scene, scenelength)


# ---------------------------------------------------------------------------------------------- the loop
def generate(geom, scene, noise, scenelength, record_scale=8, stride=2, dtype=np.float32, cg='reference'):
    """Returns dict(density [R, n, n], velocity, control [R, n, n, 2] in `dtype`, smoke [R, 8] fp64, iterations, residual per frame)."""
    st = {k: v.astype(dtype) for k, v in geom.stencil().items()}
    vmask = geom.velocity_mask.astype(dtype)
    solve = R.cg_reference if cg == 'reference' else R.cg_exact
    K = kick_frames(scene['intervals'])
    S, s = scenelength, stride
    nrec, n = S // record_scale + 1, G // s
    rec = dict(density=np.zeros((nrec, n, n), dtype), velocity=np.zeros((nrec, n, n, 2), dtype), control=np.zeros((nrec, n, n, 2), dtype),
               smoke=np.zeros((nrec, 8)), iterations=[], residual=[])
    vel = np.empty((G, G, 2), dtype)
    vel[..., 0], vel[..., 1] = dtype(0), dtype(np.float32(0.2))
    d0 = np.zeros((N, N), dtype)
    d0[scene['ys'][0]:scene['ys'][0] + 11, scene['xs'][0]:scene['xs'][0] + 11] = 1
    dens = z = d0
    outs = np.zeros(7)
    pad = lambda a: np.pad(a, ((0, 1), (0, 1)))

    def bucket_rule(z):
        arr = pad(z).astype(np.float64)
        if np.sum(arr * geom.bucket_concat) > 0:
            for i in range(7):
                outs[i] += np.sum((arr * geom.buckets[i])[::s, ::s])
            z = (z * geom.set_zero[:-1, :-1]).astype(dtype)
        return z

    for f in range(S + 1):
        kick, record, k = f in K, f % record_scale == 0, f // record_scale
        if kick:
            field = noise[f].astype(np.float32).astype(dtype)
        elif dtype == np.float32:
            field = (vel.astype(np.float64) + noise[f]).astype(np.float32)
        else:
            field = vel + noise[f]
        cur = field.copy()
        cur[16:112, 16:112] = 0
        if record:
            rec['control'][k] = cur[::s, ::s]
        cur[16:112, 16:112] = vel[16:112, 16:112]
        cur = cur * vmask
        p, it, res = solve(st, R.divergence(cur))
        vel = (cur - R.gradient(p) * vmask) * vmask
        rec['iterations'].append(it); rec['residual'].append(res)
        if f == 0:
            dens = R.advect(dens, vel)
            z = dens.copy()
        else:
            z, dens = R.advect(z, vel), R.advect(dens, vel)
            if not kick or record:
                z = bucket_rule(z)
        if record:
            rec['density'][k] = pad(dens)[::s, ::s]
            rec['velocity'][k] = vel[::s, ::s]
            if f == 0:
                rec['velocity'][k, ..., 1] = vel[::s, ::s, 0]          # a_gen_train.py:453-454
            rec['smoke'][k, :7] = outs
            rec['smoke'][k, 7] = np.sum(pad(dens if (kick or f == 0) else z).astype(np.float64)[::s, ::s])
    rec['iterations'], rec['residual'] = np.array(rec['iterations']), np.array(rec['residual'])
    return rec


def share(smoke):
    """The training quantity of data_2d.Smoke: Smoke[:, 1] / Smoke.sum(-1)."""
    smoke = np.asarray(smoke, np.float64)
    return smoke[:, 1] / smoke.sum(-1)


# ---------------------------------------------------------------------------------------------- the seeded noise source
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: Parallel random numbers: as easy as 1, 2, 3; SC'11). counter [..., 4], key [..., 2]
    uint32 (broadcast against each other) -> [..., 4] uint32."""
    c = [np.asarray(counter, np.uint32)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key, np.uint32)[..., i].astype(np.uint64) for i in range(2)]
    mask = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + np.uint64(_W0)) & mask, (k[1] + np.uint64(_W1)) & mask]
    return np.stack(np.broadcast_arrays(*c), -1).astype(np.uint32)


def unit_normals(seed, scene_index, frame):
    """The two unit normals of every cell of one frame of one scene: fp32 [128, 128, 2]. key = the 64-bit seed, counter = (cell 128 i + j,
    frame, scene_index low, scene_index high); u = ((x >> 9) + 0.5) 2^-23 of outputs 0 and 1; z = r (cos, sin)(2 pi u2),
    r = sqrt(-2 ln u1). The uniforms are exact in fp32; from there on each step is evaluated in fp64 and rounded to fp32 once, so the
    result is within an fp32 rounding or two of the exactly rounded pair."""
    seed, scene_index = int(seed) % 2 ** 64, int(scene_index) % 2 ** 64
    ctr = np.empty((G * G, 4), np.uint32)
    ctr[:, 0] = np.arange(G * G, dtype=np.uint32)
    ctr[:, 1], ctr[:, 2], ctr[:, 3] = frame, scene_index & 0xffffffff, scene_index >> 32
    x = philox4x32_10(ctr, np.array([seed & 0xffffffff, seed >> 32], np.uint32))
    u1 = ((x[:, 0] >> 9).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)
    u2 = ((x[:, 1] >> 9).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)
    r = np.sqrt((np.float32(-2) * np.log(u1.astype(np.float64)).astype(np.float32)).astype(np.float64)).astype(np.float32)
    ang = 2 * np.pi * u2.astype(np.float64)
    z = np.stack([r * np.cos(ang).astype(np.float32), r * np.sin(ang).astype(np.float32)], -1)
    return z.reshape(G, G, 2)


def noise_field(seed, scene_index, frame, kick_v=None):
    """What the seeded source delivers for a frame: 0.1 z, or on a kick v + (|v| / 10) z, in fp32."""
    z = unit_normals(seed, scene_index, frame)
    if kick_v is None:
        return np.float32(0.1) * z
    v = np.asarray(kick_v, np.float32)
    return v + (np.abs(v) / np.float32(10)) * z


# ---------------------------------------------------------------------------------------------- the reference fixtures
def load_golden():
    """(arrays, manifest) of tests/golden/ref_smoke_datagen*.npz (make_ref_smoke_datagen_golden.py)."""
    with open(os.path.join(GOLDEN, 'ref_smoke_datagen_manifest.json')) as f:
        manifest = json.load(f)
    arrays = {}
    for fn in manifest['files']:
        with np.load(os.path.join(GOLDEN, fn)) as z:
            arrays.update(R.unshuffled(k, z[k]) for k in z.files)
    return arrays, manifest


FIELDS = ('density', 'velocity', 'control', 'smoke')


def stored(arrays, name, field):
    """(reference, exact) of a case's field as float64; exact = reference + d (smoke_solver_ref.encode_exact; the smoke table in fp64)."""
    ref = arrays[f'{name}/{field}'].astype(np.float64)
    if field == 'smoke':
        return ref, ref + arrays[f'{name}/smoke_exact_d']
    return ref, ref + arrays[f'{name}/{field}_exact_d16'].astype(np.float64) * float(arrays[f'{name}/{field}_exact_scale'])


def stored_records(manifest, name, field):
    """The record numbers a case's field is stored at."""
    c = manifest['cases'][name]
    return list(range(0, c['records'], c['record_step'].get(field, 1)))
