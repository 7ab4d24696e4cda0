"""The smoke data-set generator on MI355X: the simulator behind the reference's training and test sets (smoke/dataset/a_gen_train.py,
a_gen_test_64.py, a_gen_test_128.py: exp2_target_128, get_per_vel, get_intial_state, loop_write_0423) as one launch of
csrc/smoke_datagen.hip (wdno_smoke_generate): one workgroup per scene, frames 0..scenelength, each frame's conjugate-gradient pressure
solve included. The reference runs one PhiFlow CPU process per scene (seconds to a minute each) and seeds it with its pid.

sample_scenes()  -- plain numpy: the scene parameters (turning points, kick velocities, intervals) of scene i from
                    np.random.RandomState((seed + i) % 2**32) in the reference's call order, so sample_scenes([0], S) is what the reference
                    computes after np.random.seed(S).
plan()           -- pure Python: kick frames, record count and size, the errors for shapes that cannot run, the kernel configuration.
generate()       -- one launch on torch's current stream; returns the four record tensors on the GPU.
noise_fields()   -- the fields the seeded noise source delivers (wdno_smoke_noise), for tests and for inspecting a data set's noise.
write_dataset()  -- batches of scenes to sim_%06d/{Density,Velocity,Control,Smoke}.npy, domain.npy, smoke_out.csv in the reference's
                    shapes, where ddpm/data_2d.Smoke and wave_trans_2d.py read them. read_sim() reads one back by Smoke.__getitem__'s rules.

A frame is the solver's frame (wdno_amd.smoke_solver, same device code: csrc/smoke_flow.h) with three differences: the 16-cell rim of the
velocity is not a control input but the previous frame's projected rim plus N(0, 0.1) noise, or on the scene's four kick frames
K = [0, i0, i0 + i1, i0 + i1 + i2] a fresh N(v, |v| / 10) field; the bucket rule tests the set-zero density, sums on the recorded stride
and is skipped on kick frames that are not recorded (and at frame 0); every record_scale-th frame is recorded at a spatial stride.

Arithmetic. As the solver's (fp32 fields, CG dot products pairwise, the pressure summed in fp64, fp64 interpolation weights and bucket
sums), and one step wider: the advection coordinate idx - v is formed in fp64 from the fp32 velocity, where the reference and the solver
form it in fp32 (an error of up to 3.8e-6 cells per frame near idx = 100, which a smoke front's leading edge shows).

Noise. `noise=` (explicit source) is a float64 [B, scenelength + 1, 128, 128, 2] array of what np.random.normal delivered: the N(0, 0.1)
draw on an ordinary frame, the drawn field itself on a kick frame. With the draws of the reference it reproduces the reference; it costs
67 MB per 256-frame scene and is meant for tests. `seed=` (seeded source) reads nothing: Philox4x32-10 with key = seed and counter =
(cell, frame, scene index low, high) gives two uniforms u = ((x >> 9) + 0.5) 2^-23, Box-Muller in fp32 two unit normals z, the field
is 0.1 z or v + (|v| / 10) z. The scene index is scenes['index'], the scene's number in the data set, not its batch position: a scene has
the same bits in any batch. The seeded source is by definition the explicit one fed noise_fields(...) widened to float64.

Reference quirks that are kept: record 0 of the velocity holds component 0 in both slots (a_gen_train.py:453-454); on a kick frame the
bucket rule runs only if the frame is recorded (l.581-584); Smoke[:, 7] sums the set-zero density after zeroing on an ordinary frame but
the never-zeroed density on a kick frame and at record 0 (l.574, 520, 544)."""
import argparse
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from wdno_amd import smoke_solver as _solver
from wdno_amd.smoke_solver import ACCURACY, DEFAULT_THREADS, GRID, MAX_ITER, THREADS, WS_FLOATS, check_not_forked_gpu_child, geometry

MAX_SCENELENGTH = 256
WRITERS = 8           # threads of write_dataset's one writer pool: a constant, never the machine's CPU count
# the three generators differ only in recording; `dir` is where ddpm/data_2d.Smoke looks under its dataset_path
SPLITS = {
    'train': dict(record_scale=8, stride=2, dir='train'),                        # a_gen_train.py: 33 records of 64 x 64
    'test_64': dict(record_scale=1, stride=2, dir=os.path.join('test', 'control')),      # a_gen_test_64.py: 257 records of 64 x 64
    'test_128': dict(record_scale=8, stride=1, dir=os.path.join('test', 'simulation')),  # a_gen_test_128.py: 33 records of 128 x 128
}


def _scene(rs, scenelength):
    """exp2_target_128() then get_per_vel() (a_gen_train.py:300-327, 256-297) on the RandomState rs, in their call order."""
    m = 5
    start_x = rs.randint(16 + 1 + m, 112 - 10 - m)
    start_y = rs.randint(16 + 1 + m, 40 - 10 - m)
    left = start_x < 64 - 10
    draw = (lambda: rs.randint(16 + m, 64 - 10)) if left else (lambda: rs.randint(64, 112 - 10 - m))      # only the taken branch draws
    target1_x = draw()
    target2_x = draw()
    target3_x = rs.randint(50, 80 - 1 - 10)
    end_x = rs.randint(64 - 8, 64 + 8 - 10)
    xs = [int(start_x), int(target1_x), int(target2_x), int(target3_x), int(end_x)]
    ys = [int(start_y), 40, 50, 64, 112]
    d = [((xs[k + 1] - xs[k]) ** 2 + (ys[k + 1] - ys[k]) ** 2) ** 0.5 for k in range(4)]
    distance = d[0] + d[1] + d[2] + d[3]
    v = distance / float(scenelength)
    vx = [v * (xs[k + 1] - xs[k]) / d[k] for k in range(4)]
    vy = [v * (ys[k + 1] - ys[k]) / d[k] for k in range(4)]
    scale = rs.uniform(2, 5)
    real_vel = lambda vel: rs.normal(vel, abs(vel / 4))                  # get_real_vel
    vxs = [real_vel(scale * c) for c in vx]
    vys = [real_vel(5 * c) for c in vy]
    intervals = [int(scenelength * d[k] / distance) for k in range(3)]
    return xs, ys, vxs, vys, intervals


def sample_scenes(scene_indices, seed, scenelength=256):
    """Scene parameters of the given scene numbers of data set `seed`: dict(index [B] int64, xs, ys [B, 5] int64, vxs, vys [B, 4]
    float64, intervals [B, 3] int64, scenelength). Scene i draws from np.random.RandomState((seed + i) % 2**32)."""
    idx = np.asarray(list(scene_indices), np.int64).reshape(-1)
    rows = [_scene(np.random.RandomState(int((int(seed) + int(i)) % 2 ** 32)), scenelength) for i in idx]
    col = lambda k, dt: np.array([r[k] for r in rows], dt).reshape(len(rows), -1)
    return dict(index=idx, xs=col(0, np.int64), ys=col(1, np.int64), vxs=col(2, np.float64), vys=col(3, np.float64),
                intervals=col(4, np.int64), scenelength=int(scenelength))


def kick_frames(intervals):
    """K = [0, i0, i0 + i1, i0 + i1 + i2] per scene: [B, 4] int64."""
    iv = np.asarray(intervals, np.int64).reshape(-1, 3)
    return np.concatenate([np.zeros((iv.shape[0], 1), np.int64), np.cumsum(iv, 1)], 1)


def plan(scenes, record_scale=8, stride=2, threads=None):
    """Host integers of one call: dict(B, scenelength, record_scale, stride, kick_frames [B, 4], records R, n, threads, max_iter,
    accuracy). Raises ValueError for what cannot run: scenelength outside [1, 256], record_scale < 1, a stride not in {1, 2}, an interval
    below 1 (the reference's loop is ill-defined there), a density block outside the grid, an unsupported `threads`."""
    S = int(scenes['scenelength'])
    if not 1 <= S <= MAX_SCENELENGTH:
        raise ValueError(f'smoke datagen: scenelength {S} is outside [1, {MAX_SCENELENGTH}]')
    record_scale, stride = int(record_scale), int(stride)
    if record_scale < 1:
        raise ValueError(f'smoke datagen: record_scale {record_scale} < 1')
    if stride not in (1, 2):
        raise ValueError(f'smoke datagen: stride {stride} is not 1 or 2')
    iv = np.asarray(scenes['intervals'], np.int64).reshape(-1, 3)
    B = iv.shape[0]
    if B == 0:
        raise ValueError('smoke datagen: no scenes')
    if iv.min() < 1:
        raise ValueError(f'smoke datagen: interval {int(iv.min())} < 1 (scene {int(np.asarray(scenes["index"])[np.argmin(iv.min(1))])}): '
                         'the reference\'s loop is ill-defined for it')
    K = kick_frames(iv)
    if K.max() > S:
        raise ValueError(f'smoke datagen: kick frame {int(K.max())} beyond scenelength {S}')
    xs0, ys0 = np.asarray(scenes['xs'])[:, 0], np.asarray(scenes['ys'])[:, 0]
    if min(xs0.min(), ys0.min()) < 0 or max(xs0.max(), ys0.max()) + 11 > GRID - 1:
        raise ValueError('smoke datagen: the 11 x 11 block of initial density leaves the 127 x 127 grid')
    for k in ('index', 'xs', 'ys', 'vxs', 'vys'):
        if np.asarray(scenes[k]).shape[0] != B:
            raise ValueError(f'smoke datagen: scenes[{k!r}] has {np.asarray(scenes[k]).shape[0]} rows for {B} scenes')
    threads = DEFAULT_THREADS if threads is None else int(threads)
    if threads not in THREADS:
        raise ValueError(f'smoke datagen: {threads} threads per scene is not a supported configuration: {THREADS}')
    return dict(B=B, scenelength=S, record_scale=record_scale, stride=stride, kick_frames=K, records=S // record_scale + 1, n=GRID // stride,
                threads=threads, max_iter=MAX_ITER, accuracy=float(np.float32(ACCURACY)))


def _scene_tables(scenes, pl, dev):
    B = pl['B']
    si = np.zeros((B, 8), np.int32)
    si[:, 0], si[:, 1], si[:, 2:6] = np.asarray(scenes['xs'])[:, 0], np.asarray(scenes['ys'])[:, 0], pl['kick_frames']
    sv = np.zeros((B, 8), np.float32)
    sv[:, 0::2], sv[:, 1::2] = np.asarray(scenes['vxs'], np.float64), np.asarray(scenes['vys'], np.float64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t(si), t(sv), t(np.asarray(scenes['index'], np.int64))


def generate(scenes, seed=None, noise=None, record_scale=8, stride=2, threads=None, geom=None):
    """The reference's get_intial_state + loop_write_0423 for the scenes of sample_scenes() (or a dict of the same arrays), in one launch
    on the current stream. Exactly one of `seed` (seeded noise source) and `noise` (explicit: float64 [B, scenelength + 1, 128, 128, 2],
    numpy or tensor) is given. Returns (density [B, R, n, n], velocity [B, R, n, n, 2], control [B, R, n, n, 2]) fp32 and smoke [B, R, 8]
    fp64 on the current GPU, R = scenelength // record_scale + 1, n = 128 // stride."""
    check_not_forked_gpu_child('wdno_amd.smoke_datagen.generate')
    if (seed is None) == (noise is None):
        raise ValueError('smoke datagen: give exactly one of seed= (seeded noise source) and noise= (explicit noise)')
    from wdno_amd import _lib
    pl = plan(scenes, record_scale, stride, threads)
    geom = geometry() if geom is None else geom
    B, S, R, n = pl['B'], pl['scenelength'], pl['records'], pl['n']
    dev = torch.device('cuda', torch.cuda.current_device())
    lib = _lib.load()
    with torch.no_grad(), torch.cuda.device(dev):
        if noise is not None:
            noise = torch.as_tensor(noise)
            if tuple(noise.shape) != (B, S + 1, GRID, GRID, 2) or noise.dtype != torch.float64:
                raise ValueError(f'smoke datagen: noise must be float64 [{B}, {S + 1}, {GRID}, {GRID}, 2], got {noise.dtype} {tuple(noise.shape)}')
            noise = noise.to(dev).contiguous()
        si, sv, index = _scene_tables(scenes, pl, dev)
        v0 = torch.from_numpy(_solver.init_velocity(0.0, 0.2)).to(dev).reshape(GRID, GRID, 2).contiguous()
        fluid, active, vmask, buckets = geom.device_masks(dev)
        density = torch.empty(B, R, n, n, device=dev, dtype=torch.float32)
        velocity = torch.empty(B, R, n, n, 2, device=dev, dtype=torch.float32)
        control = torch.empty(B, R, n, n, 2, device=dev, dtype=torch.float32)
        smoke = torch.empty(B, R, 8, device=dev, dtype=torch.float64)
        ws = torch.empty(B, WS_FLOATS, device=dev, dtype=torch.float32)
        desc = _lib.SmokeGenerateDesc(B=B, scenelength=S, record_scale=pl['record_scale'], stride=pl['stride'], max_iter=pl['max_iter'],
                                      threads=pl['threads'], noise_mode=0 if noise is not None else 1, accuracy=pl['accuracy'],
                                      seed=0 if seed is None else int(seed) % 2 ** 64)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.wdno_smoke_generate(si.data_ptr(), sv.data_ptr(), index.data_ptr(), noise.data_ptr() if noise is not None else None,
                                           v0.data_ptr(), fluid.data_ptr(), active.data_ptr(), vmask.data_ptr(), buckets.data_ptr(),
                                           density.data_ptr(), velocity.data_ptr(), control.data_ptr(), smoke.data_ptr(), ws.data_ptr(), desc,
                                           stream), 'wdno_smoke_generate')
    return density, velocity, control, smoke


def noise_fields(scenes, seed, frames):
    """The fields the seeded source delivers to the given scenes at the given frames: fp32 [B, len(frames), 128, 128, 2] on the current GPU
    (0.1 z on an ordinary frame, v + (|v| / 10) z on one of the scene's kick frames)."""
    check_not_forked_gpu_child('wdno_amd.smoke_datagen.noise_fields')
    from wdno_amd import _lib
    frames = [int(f) for f in frames]
    K = kick_frames(scenes['intervals'])
    B, F = K.shape[0], len(frames)
    if not F or min(frames) < 0 or max(frames) > int(scenes['scenelength']):
        raise ValueError('smoke datagen: frames must lie in [0, scenelength]')
    idx = np.repeat(np.asarray(scenes['index'], np.int64), F)
    fr = np.tile(np.asarray(frames, np.int32), B)
    is_kick = np.zeros(B * F, np.int32)
    kv = np.zeros((B * F, 2), np.float32)
    for b in range(B):
        for j, f in enumerate(frames):
            hit = np.nonzero(K[b] == f)[0]
            if hit.size:
                k = int(hit[-1])
                is_kick[b * F + j] = 1
                kv[b * F + j] = (scenes['vxs'][b][k], scenes['vys'][b][k])
    dev = torch.device('cuda', torch.cuda.current_device())
    lib = _lib.load()
    out = torch.empty(B, F, GRID, GRID, 2, device=dev, dtype=torch.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    idx_d, fr_d, ik_d, kv_d = t(idx), t(fr), t(is_kick), t(kv)
    step = 65535
    for a in range(0, B * F, step):
        m = min(step, B * F - a)
        _lib.check(lib.wdno_smoke_noise(idx_d[a:].data_ptr(), fr_d[a:].data_ptr(), ik_d[a:].data_ptr(), kv_d[a:].data_ptr(), m,
                                        int(seed) % 2 ** 64, out.view(B * F, GRID, GRID, 2)[a:].data_ptr(),
                                        torch.cuda.current_stream(dev).cuda_stream), 'wdno_smoke_noise')
    return out


# ---------------------------------------------------------------------------------------------- files
def sim_dir(root, scene_index):
    return os.path.join(root, f'sim_{int(scene_index):06d}')


def write_sim(path, density, velocity, control, smoke, domain, dtype=np.float64):
    """One scene's files in the reference's shapes: Density [n, n, 1, R], Velocity, Control [n, n, 2, R], Smoke [R, 8] (`dtype`; the
    values are fp32-exact, Smoke is always float64), domain.npy (the active mask, [1, 127, 127, 1]) and smoke_out.csv."""
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, 'Density.npy'), np.ascontiguousarray(np.moveaxis(density, 0, -1)[:, :, None, :], dtype=dtype))
    np.save(os.path.join(path, 'Velocity.npy'), np.ascontiguousarray(velocity.transpose(1, 2, 3, 0), dtype=dtype))
    np.save(os.path.join(path, 'Control.npy'), np.ascontiguousarray(control.transpose(1, 2, 3, 0), dtype=dtype))
    np.save(os.path.join(path, 'Smoke.npy'), np.asarray(smoke, np.float64))
    np.save(os.path.join(path, 'domain.npy'), domain)
    np.savetxt(os.path.join(path, 'smoke_out.csv'), np.asarray(smoke, np.float64), delimiter=',')


def read_sim(root, scene_index, steps=32):
    """A scene read back by the rules of ddpm/data_2d.Smoke.__getitem__ (the loader the reference trains on): Density, Velocity, Control
    permuted (2, 3, 0, 1), the smoke share Smoke[:, 1] / Smoke.sum(-1) broadcast over the cells, concatenated to 6 channels, the first
    `steps` records -> fp32 [steps, 6, n, n] (not rescaled)."""
    path = sim_dir(root, scene_index)
    d, v, c = (torch.tensor(np.load(os.path.join(path, f + '.npy')), dtype=torch.float).permute(2, 3, 0, 1) for f in ('Density', 'Velocity', 'Control'))
    s = torch.tensor(np.load(os.path.join(path, 'Smoke.npy')), dtype=torch.float)
    s = s[:, 1] / s.sum(-1)
    s = s.reshape(1, s.shape[0], 1, 1).expand(1, s.shape[0], d.shape[-2], d.shape[-1])
    return torch.cat((d, v, c, s), dim=0)[:, :steps].permute(1, 0, 2, 3)


def write_scenes(path, scene_indices, seed, record_scale=8, stride=2, scenelength=256, batch=256, dtype=np.float64, threads=None, geom=None):
    """Generates the scenes in batches and writes them under `path`/sim_%06d. The device-to-host copy (on a side stream, into pinned
    memory) and the file writes of batch k run while batch k + 1 is on the GPU; one pool of WRITERS threads does the writes. Returns the
    number of scenes written."""
    check_not_forked_gpu_child('wdno_amd.smoke_datagen.write_scenes')
    geom = geometry() if geom is None else geom
    idx = [int(i) for i in scene_indices]
    domain = np.ascontiguousarray(geom._active_mask)
    dev = torch.device('cuda', torch.cuda.current_device())
    copy_stream = torch.cuda.Stream(dev)
    pending, written = [], []          # (host tensors, copy-done event, scene numbers) of the batch on its way; futures of earlier batches

    def flush(item):
        host, done, ids = item
        done.synchronize()
        arrays = [h.numpy() for h in host]
        for b, i in enumerate(ids):
            written.append(pool.submit(write_sim, sim_dir(path, i), arrays[0][b], arrays[1][b], arrays[2][b], arrays[3][b], domain, dtype))

    with ThreadPoolExecutor(max_workers=WRITERS) as pool:
        for a in range(0, len(idx), int(batch)):
            ids = idx[a:a + int(batch)]
            out = generate(sample_scenes(ids, seed, scenelength), seed=seed, record_scale=record_scale, stride=stride, threads=threads, geom=geom)
            ready = torch.cuda.current_stream(dev).record_event()
            if pending:
                flush(pending.pop())          # batch k: its copy and writes overlap batch k + 1, launched above
            copy_stream.wait_event(ready)
            with torch.cuda.stream(copy_stream):
                host = [torch.empty(o.shape, dtype=o.dtype, pin_memory=True).copy_(o, non_blocking=True) for o in out]
                for o in out:
                    o.record_stream(copy_stream)
                done = copy_stream.record_event()
            pending.append((host, done, ids))
            while len(written) > 2 * int(batch):          # bound what waits for the disk
                written.pop(0).result()
        if pending:
            flush(pending.pop())
        for f in written:
            f.result()
    return len(idx)


def write_dataset(root, split, scene_range, seed, batch=256, dtype=np.float64, scenelength=256, threads=None):
    """The scenes scene_range (a range or a sequence of scene numbers) of data set `seed` for split 'train', 'test_64' or 'test_128', under
    root/train, root/test/control or root/test/simulation -- where data_2d.Smoke(dataset_path=root) and wave_trans_2d.py read them. dtype
    np.float32 halves the files (the values are fp32-exact either way; the full float64 training set is 108 GB)."""
    if split not in SPLITS:
        raise ValueError(f'smoke datagen: split {split!r} is not one of {sorted(SPLITS)}')
    sp = SPLITS[split]
    return write_scenes(os.path.join(root, sp['dir']), scene_range, seed, sp['record_scale'], sp['stride'], scenelength, batch, dtype, threads)


# ---------------------------------------------------------------------------------------------- the reference's scripts
# (scenes per branch for Test_ / is_train / neither, the directory a Test_ run writes to) of a_gen_train.py:707-736 and its twins
_SCRIPTS = {
    'train': ((5, 2, 40), 'test_0501'),
    'test_64': ((10, 5, 40), 'test0506_256_64_64'),
    'test_128': ((5, 40, 40), 'test0507_32_128_128'),
}


def branch_scenes(split, is_train_, Test_, branch_num):
    """The scene numbers the reference's exp2_same_side_128 generates for a branch: scenecount * branch .. scenecount * (branch + 1)."""
    counts, _ = _SCRIPTS[split]
    count = counts[0] if Test_ else (counts[1] if is_train_ else counts[2])
    return range(count * int(branch_num), count * (int(branch_num) + 1))


def exp2_same_side_128(split, is_train_, fix_velocity_, Test_, branch_num, data_savepath, seed=0, batch=256):
    """exp2_same_side_128 of the reference's generator for `split`: the same scene numbers per branch, the same directory
    (./<data_savepath>/, or the script's fixed directory when Test_) and files. The reference seeds numpy with its pid and draws its
    scenes one after another from that stream; here scene i is scene i of data set `seed`, whatever branch or batch generates it."""
    path = _SCRIPTS[split][1] if Test_ else f'./{data_savepath}/'
    sp = SPLITS[split]
    n = write_scenes(path, branch_scenes(split, is_train_, Test_, branch_num), seed, sp['record_scale'], sp['stride'], batch=batch)
    print('DATA GENERATION DOWN!')
    return n


def script_main(split, argv=None):
    """The reference's command line (--test_or_train --data_savepath --branch_begin --branch_end) plus --seed; one process, the
    branches one after another (no multiprocessing.Pool: a GPU process is not forked)."""
    ap = argparse.ArgumentParser()
    ap.add_argument('--test_or_train', type=str, help='(test:input test or train)')
    ap.add_argument('--data_savepath', type=str, help='dataset location')
    ap.add_argument('--branch_begin', type=str, help='branch begin number')
    ap.add_argument('--branch_end', type=str, help='branch end number')
    ap.add_argument('--seed', type=int, default=0, help='data-set seed (the reference seeds with its pid)')
    args = ap.parse_args(argv)
    if args.test_or_train not in ('test', 'train'):
        raise SystemExit('--test_or_train must be test or train')
    Test_ = args.test_or_train == 'test'
    for branch in range(int(args.branch_begin), int(args.branch_end)):
        exp2_same_side_128(split, not Test_, False, Test_, str(branch), args.data_savepath, seed=args.seed)


def main(argv=None):
    ap = argparse.ArgumentParser(description='Generate smoke scenes on the GPU in the reference\'s file layout.')
    ap.add_argument('--split', choices=sorted(SPLITS), required=True)
    ap.add_argument('--data_savepath', required=True, help='data set root (the dataset_path of data_2d.Smoke)')
    ap.add_argument('--scenes', required=True, help='A:B, scene numbers A..B-1')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--dtype', choices=('float64', 'float32'), default='float64')
    args = ap.parse_args(argv)
    a, b = (int(v) for v in args.scenes.split(':'))
    n = write_dataset(args.data_savepath, args.split, range(a, b), args.seed, batch=args.batch, dtype=np.dtype(args.dtype).type)
    print(f'{n} scenes of split {args.split} written under {os.path.join(args.data_savepath, SPLITS[args.split]["dir"])}')


if __name__ == '__main__':
    main()
