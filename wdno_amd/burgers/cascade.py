"""The hand-off between two levels of the zero-shot super-resolution cascade on the GPU: what evaluate (eval_ddpm_burgers.py:306-338) hands
to the super model's sample() as low, u_init and u_final, written as the sampler's condition source [B, 17, P_t, P_x] in network units by one
launch of csrc/burgers_cascade.hip (include/wdno_hip.h: wdno_burgers_cascade_conditions), which writes every element of the source.

The reference builds these with upsample_coef (an expand and a copying reshape), a pad, a division, a second get_target (which re-reads
and re-slices the test file, transforms two rows and fills a zeroed tensor), two slices and two divisions and, inside sample(), three copies
into a zeroed tensor. Here the previous level's block and the two target rows are read in place through their strides, the nearest x2, the
1-D analysis, the zero padding and the divisions happen in the store, and GaussianDiffusion.sample_with_source(src, ...) takes the tensor
as it is.

super_conditions() -- on GPU tensors the launch, on torch's current stream; on CPU tensors the same values in plain torch (the route of the
                      CPU tests); (wave, mode) pairs the kernel is not built for take the plain-torch formulation on this tree's operators.
views()            -- (low, u_init, u_final) as views of the source, for sample(low=, u_init=, u_final=) and sample_with_source.
plan()             -- pure Python: the descriptor's integers and the grid; needs neither the library nor a GPU.
get_target_view(), super_shapes(), load_super_model() -- what the driver needs around the launch: the level's target as a strided
                      view of the held test file, the levels' shape lists, and the 17-channel model loaded from args.super_checkpoint.

Rows of low. The fine block (h1, w1) has an odd height (81, 161, ...), and twice the previous block is one row more (82 against 81): the
reference copies ps[0] + 1 rows of low into the state (diffusion_1d.py: _sampling_setup), and so does this.
"""
import ctypes as C

import torch

from wdno_amd.burgers.guidance import SUPPORTED

CHANNELS = 17
TILE = 16            # rows of a plane a workgroup stores: 8 KB at P_x = 128, 6 800 workgroups at batch 50


def views(src):
    """(low [B, 8, P_t, P_x], u_init [B, P_t / 2, P_x], u_final [B, P_t / 2, P_x]) of a condition source."""
    half = src.shape[-2] // 2
    return src[:, 8:16], src[:, -1, :half], src[:, -1, -half:]


def plan(prev_shape, target_shape, shape1, pad_t, pad_x, is_condition_u0=True, is_condition_uT=True, wave_type='bior2.4',
         pad_mode='periodization', strides=None, target_strides=None):
    """Host integers of one wdno_burgers_cascade_conditions call: the previous level's block of prev_shape = (B, 8, h0, w0) with element
    `strides` (default: contiguous), the level's target of target_shape = (B, n_t, >= n_x) with `target_strides` = (sample, row, column),
    the fine block shape1 = (h1, w1); n_x = 2 w1 columns of the target are read. ValueError for whatever the kernel cannot walk."""
    from wdno_amd.filters import filter_bank
    if (wave_type, pad_mode) not in SUPPORTED:
        raise ValueError(f'burgers cascade conditions: (wave, mode) = ({wave_type!r}, {pad_mode!r}) is not built; supported: {sorted(SUPPORTED)}')
    L = len(filter_bank(wave_type)[0])
    B, C0, h0, w0 = (int(v) for v in prev_shape)
    Bt, n_t, n_cols = (int(v) for v in target_shape)
    h1, w1 = int(shape1[-2]), int(shape1[-1])
    pad_t, pad_x = int(pad_t), int(pad_x)
    n_x = 2 * w1
    if C0 != 8:
        raise ValueError(f'burgers cascade conditions: the previous block has {C0} channels; the 8 coefficient channels are handed on')
    if Bt != B or B < 1 or B > 65535:
        raise ValueError(f'burgers cascade conditions: a block of {B} and a target of {Bt} samples; one batch of 1 .. 65535 is needed')
    if pad_t < 4 or pad_t % 4 or pad_x < 4 or pad_x % 4 or pad_x > 2048 or CHANNELS * pad_t * pad_x >= 2 ** 31:
        raise ValueError(f'burgers cascade conditions: P_t = {pad_t} and P_x = {pad_x} must be multiples of 4 (four stripes; 16-byte rows), '
                         'P_x at most 2048 and a sample inside 32 bits')
    if h0 < 1 or w0 < 1 or 2 * h0 != h1 + 1 or 2 * w0 != w1:
        raise ValueError(f'burgers cascade conditions: twice the previous block {(h0, w0)} is not the fine block {(h1, w1)} plus one row')
    if 2 * h0 > pad_t or 2 * w0 > pad_x:
        raise ValueError(f'burgers cascade conditions: the up-sampled block {(2 * h0, 2 * w0)} does not fit ({pad_t}, {pad_x})')
    if n_t < 2 or n_x < L or n_cols < n_x:
        raise ValueError(f'burgers cascade conditions: a target of {n_t} rows and {n_cols} columns; rows 0 and -1 of {n_x} >= {L} columns are read')
    ss, cs, rs, es = (8 * h0 * w0, h0 * w0, w0, 1) if strides is None else (int(v) for v in strides)
    tss, trs, tcs = (n_t * n_cols, n_cols, 1) if target_strides is None else (int(v) for v in target_strides)
    if es != 1 or rs < w0 or cs < h0 * rs or ss < 8 * cs or cs >= 2 ** 31:
        raise ValueError(f'burgers cascade conditions: strides {(ss, cs, rs, es)} of a {tuple(prev_shape)} block: columns must be contiguous and '
                         'the axes nested in the order sample, channel, row')
    if tss < 0 or trs < 0 or tcs < 1:
        raise ValueError(f'burgers cascade conditions: target strides {(tss, trs, tcs)} are outside what the kernel walks')
    tile = min(TILE, pad_t)
    ntile = -(-pad_t // tile)
    return dict(prev_sample_stride=ss, tgt_sample_stride=tss, tgt_row_stride=trs, tgt_col_stride=tcs, prev_chan_stride=cs, prev_row_stride=rs,
                B=B, C=CHANNELS, h0=h0, w0=w0, h1=h1, w1=w1, n_t=n_t, n_x=n_x, P_t=pad_t, P_x=pad_x, tile=tile, ntile=ntile,
                cond_u0=int(bool(is_condition_u0)), cond_uT=int(bool(is_condition_uT)), L=L, mode=0, lds_bytes=16 * pad_x, reserved=0,
                grid=(ntile, CHANNELS, B))


# ----------------------------------------------------------------------------------------------------- plain torch
def _analysis_rows(rows, wave_type, pad_mode):
    """(lo, hi) [B, 2, n_x / 2] of rows [B, 2, n_x]: on the GPU this tree's DWT1DForward; on the CPU the periodized sums written out, fp32,
    m = 0 .. L - 1: y[k] = sum_m dec[L - 1 - m] x[(2 k + m - (L / 2 - 1)) mod n_x]."""
    if rows.is_cuda:
        from wdno_amd import wavelets as W
        lo, hi = W.DWT1DForward(J=1, mode=pad_mode, wave=wave_type)(rows.contiguous())
        return lo, hi[0]
    from wdno_amd.filters import filter_bank
    if pad_mode not in ('periodization', 'per') or rows.shape[-1] % 2:
        raise ValueError(f'burgers cascade conditions: the CPU route takes periodization on an even width, got {pad_mode!r} on {rows.shape[-1]}')
    dl, dh = filter_bank(wave_type)[:2]
    L, n_x = len(dl), rows.shape[-1]
    k2 = 2 * torch.arange(n_x // 2)
    lo = torch.zeros(rows.shape[:-1] + (n_x // 2,), dtype=rows.dtype)
    hi = torch.zeros_like(lo)
    for m in range(L):
        v = rows[..., (k2 + m - (L // 2 - 1)) % n_x]
        lo = lo + torch.tensor(float(dl[L - 1 - m]), dtype=rows.dtype) * v
        hi = hi + torch.tensor(float(dh[L - 1 - m]), dtype=rows.dtype) * v
    return lo, hi


def _torch_conditions(x_prev, u_target, r, shape1, pad_t, pad_x, cond_u0, cond_uT, wave_type, pad_mode):
    B, h0, w0 = x_prev.shape[0], x_prev.shape[2], x_prev.shape[3]
    n_x = 2 * int(shape1[-1])
    src = torch.zeros(B, CHANNELS, pad_t, pad_x, dtype=torch.float32, device=x_prev.device)
    low = x_prev.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    src[:, 8:16, :2 * h0, :2 * w0] = low / r[8:16].reshape(1, 8, 1, 1)
    lo, hi = _analysis_rows(u_target[:, [0, -1], :n_x], wave_type, pad_mode)
    nx, rep = lo.shape[-1], pad_t // 4
    if cond_u0:
        src[:, -1, :rep, :nx] = (lo[:, [0]] / r[-1])
        src[:, -1, rep:2 * rep, :nx] = (hi[:, [0]] / r[-1])
    if cond_uT:
        src[:, -1, 2 * rep:3 * rep, :nx] = (lo[:, [1]] / r[-1])
        src[:, -1, 3 * rep:, :nx] = (hi[:, [1]] / r[-1])
    return src


# ----------------------------------------------------------------------------------------------------- the level's target, shapes and model
# These live here and not in ddpm_burgers/test_util.py: that drop-in stays as it is, and its load_2dconv_super_model keeps refusing. The
# driver binds load_super_model to the reference's name (eval_ddpm_burgers.load_2dconv_super_model).
def get_target_view(args, target_i, N_upsample=0, device=0, dataset='free_u_f_1e5'):
    """u of the targets target_i at level N_upsample, [n, 80 2^N + 1, 120 2^N], not rescaled, as a VIEW of the test file that
    ddpm_burgers.test_util holds: the ::step slicing of get_burgers_preprocess is a row and a column stride here, not a copy, when
    target_i is an int or a run of consecutive indices (evaluate()'s batches); any other index list is gathered. Its values are
    get_target(is_wave=False)'s without the column padding."""
    from ddpm_burgers import test_util as TU
    # test_util's holder of the test file (no public name returns the file unsliced): read on first use, found held afterwards; .db is
    # the file's dictionary on the GPU
    u = TU._test_dataset(f'data/{args.dataset}_super/test', N_upsample, device, {}).db['u']
    st, sx = int((u.shape[-2] - 1) / 80 / 2 ** N_upsample), int(u.shape[-1] / 120 / 2 ** N_upsample)
    idx = [int(target_i)] if isinstance(target_i, int) else [int(i) for i in target_i]
    if idx == list(range(idx[0], idx[0] + len(idx))):
        return u[idx[0]:idx[0] + len(idx), ::st, ::sx]
    return u[idx][:, ::st, ::sx]


def super_shapes(shape_init, ori_shape_init, upsample_x):
    """The coefficient blocks and field sizes of the levels 1 .. upsample_x (test_util.py:243-248): from (41, 60) and (81, 120),
    [[81, 120], [161, 240], ...] and [[161, 240], [321, 480], ...]."""
    grow = lambda n, i: 2 ** i * 2 * (int(n) // 2) + int(n) % 2
    shape = [[grow(shape_init[-2], i), grow(shape_init[-1], i)] for i in range(1, upsample_x + 1)]
    ori_shape = [[grow(ori_shape_init[-2], i), grow(ori_shape_init[-1], i)] for i in range(1, upsample_x + 1)]
    return shape, ori_shape


def load_super_model(model_i, args, RESCALER):
    """The super model of test_util.py:235-264 (load_2dconv_super_model there), for eval_ddpm_burgers.evaluate: the data set gives the base
    shapes, the levels' shape lists follow from them, the model is built with dim = args.super_dim, a Trainer loads args.super_checkpoint.
    The reference leaves args.dim = args.super_dim on the caller's namespace, so that the next evaluate() of its wfs x wus loop builds the
    BASE model with super_dim and fails to load its checkpoint whenever the two differ; here args.dim is put back."""
    import os
    if not args.is_super_model:
        raise NotImplementedError('wdno_amd burgers evaluation: load_2dconv_super_model needs args.is_super_model; the reference asserts it '
                                  '(reference burgers/ddpm_burgers/test_util.py:236)')
    if not args.is_wavelet:
        raise NotImplementedError('wdno_amd burgers evaluation: is_wavelet=False is not provided here '
                                  '(reference burgers/ddpm_burgers/test_util.py:239-240)')
    from ddpm_burgers import test_util as TU
    from ddpm_burgers.train_diffusion import Trainer
    dataset = TU.load_burgers_dataset_wavelet(args, RESCALER)
    shape, ori_shape = super_shapes(dataset.shape, dataset.ori_shape, args.upsample_x)
    dim = args.dim
    args.dim = args.super_dim
    try:
        ddpm = TU.get_2d_ddpm(shape, ori_shape, args, RESCALER, is_super_model=True, upsample_t=args.upsample_t, upsample_x=args.upsample_x)
    finally:
        args.dim = dim
    # (a list of one data set: this tree's Trainer draws a super model's batches from a list of levels; the loader is never used here)
    trainer = Trainer(ddpm, [dataset], is_super_model=True, wave_type=args.wave_type, pad_mode=args.pad_mode, rescaler=RESCALER,
                      results_folder=os.path.join(args.results_folder, model_i), train_num_steps=args.train_num_steps,
                      save_and_sample_every=args.checkpoint_interval)
    trainer.load(args.super_checkpoint if 'checkpoint' in args.__dict__ else 10)
    return ddpm


_filt = {}


def super_conditions(x_prev, u_target_k, rescaler, shape1, pad_t, pad_x, is_condition_u0=True, is_condition_uT=True, wave_type='bior2.4',
                     pad_mode='periodization'):
    """The condition source [B, 17, pad_t, pad_x] (fp32, network units) of a super level. x_prev [B, 8, h0, w0]: the block the previous
    level's diffuse_2dconv returned (the sample times RESCALER; a view whose columns are contiguous is read in place); u_target_k
    [B, n_t, >= 2 w1]: the level's target, not rescaled (any view with non-negative strides is read in place; rows 0 and -1 are read);
    rescaler: the 17 values in any shape; shape1 = (h1, w1): the level's coefficient block. See views()."""
    r = torch.as_tensor(rescaler, dtype=torch.float32).reshape(-1)
    if r.numel() != CHANNELS:
        raise ValueError(f'burgers cascade conditions: RESCALER has {r.numel()} entries, the super model {CHANNELS} channels')
    if x_prev.dim() != 4 or u_target_k.dim() != 3 or x_prev.dtype != torch.float32 or u_target_k.dtype != torch.float32 or \
            x_prev.device != u_target_k.device:
        raise ValueError(f'burgers cascade conditions: block {tuple(x_prev.shape)} {x_prev.dtype} on {x_prev.device} against target '
                         f'{tuple(u_target_k.shape)} {u_target_k.dtype} on {u_target_k.device}: float32 tensors on one device are needed')
    shape1 = (int(shape1[-2]), int(shape1[-1]))
    prev, tgt = x_prev.detach(), u_target_k.detach()
    B = int(prev.shape[0])
    st = list(prev.stride())
    tst = list(tgt.stride())
    if B == 1:                                     # the stride of a one-sample axis is never walked
        st[0], tst[0] = 8 * st[1], 0
    r = r.to(prev.device).contiguous()
    if not prev.is_cuda or (wave_type, pad_mode) not in SUPPORTED:
        plan(tuple(prev.shape), tuple(tgt.shape), shape1, pad_t, pad_x, is_condition_u0, is_condition_uT, strides=None)      # the sizes, on every route
        return _torch_conditions(prev, tgt, r, shape1, int(pad_t), int(pad_x), is_condition_u0, is_condition_uT, wave_type, pad_mode)
    try:
        pl = plan(tuple(prev.shape), tuple(tgt.shape), shape1, pad_t, pad_x, is_condition_u0, is_condition_uT, wave_type, pad_mode, st, tst)
    except ValueError:
        if prev.is_contiguous() and tgt.is_contiguous():
            raise
        prev, tgt = prev.contiguous(), tgt.contiguous()       # views the kernel cannot walk: one copy each
        pl = plan(tuple(prev.shape), tuple(tgt.shape), shape1, pad_t, pad_x, is_condition_u0, is_condition_uT, wave_type, pad_mode)
    from wdno_amd import _lib
    from wdno_amd.filters import filter_bank
    from wdno_amd.ops import _p, _stream
    pl.pop('grid')
    filt = _filt.get(wave_type)
    if filt is None:
        vals = [float(v) for bank in filter_bank(wave_type) for v in bank]
        filt = _filt[wave_type] = (C.c_float * len(vals))(*vals)
    with torch.cuda.device(prev.device):
        src = torch.empty((B, CHANNELS, int(pad_t), int(pad_x)), dtype=torch.float32, device=prev.device)
        desc = _lib.BurgersCascadeDesc(**pl)
        _lib.check(_lib.load().wdno_burgers_cascade_conditions(_p(prev), _p(tgt), _p(r), _p(src), C.byref(desc), filt, _stream()),
                   'wdno_burgers_cascade_conditions')
    return src
