"""The fields of a sampled Burgers state on the GPU: the wavelet branch of diffuse_2dconv (eval_ddpm_burgers.py:185-195) as one launch of
csrc/burgers_reconstruct.hip (include/wdno_hip.h: wdno_burgers_reconstruct).

The reference multiplies the sample by RESCALER, unpacks it (tensor_to_coef: four slices and two stacks), runs the IDWT and crops twice.
Here the coefficients are read in place through x's strides, the product with RESCALER is formed on the fly, and u [B, n_t, n_x] and
f [B, n_t - 1, n_x] are written once.

reconstruct() -- the launch, on torch's current stream; (wave, mode) pairs the kernel is not built for take wdno_amd.wavelets.DWTInverse.
plan()        -- pure Python: the descriptor's integers, the tile and its LDS bytes; needs neither the library nor a GPU.

Tile rule. A workgroup owns tn reconstruction rows (even) of one field at full width and keeps (lo_w, hi_w) [2][tn][w] in LDS: 8 tn w bytes.
The H pass reads the coefficients from global memory, so a tile has no halo and narrow tiles repeat nothing; tn is the largest even value
<= 32 whose buffer fits 64 KiB, re-balanced so that the tiles are equal: the evaluation's 41 x 60 block gives 3 tiles of 28 rows at 13 440 B,
6 workgroups a sample, 300 at the batch of 50 on 256 compute units.
"""
import ctypes as C

import torch

from wdno_amd.burgers.guidance import LDS_BUDGET, SUPPORTED

TILE_MAX = 32


def lds_bytes(w, tn):
    """LDS of a workgroup: (lo_w, hi_w) of its tn rows."""
    return 4 * 2 * tn * w


def plan(x_shape, shape, ori_shape, wave_type='bior2.4', pad_mode='periodization', strides=None):
    """Host integers of one wdno_burgers_reconstruct call on x of x_shape = (B, C, H, W) with element `strides` (default: contiguous).
    ValueError for a (wave, mode) the kernel is not built for, a block larger than the tensor, a crop larger than the reconstruction,
    strides the kernel cannot walk, and a block whose two-row tile does not fit the LDS budget."""
    from wdno_amd.filters import filter_bank
    if (wave_type, pad_mode) not in SUPPORTED:
        raise ValueError(f'burgers reconstruction kernel: (wave, mode) = ({wave_type!r}, {pad_mode!r}) is not built; supported: {sorted(SUPPORTED)}')
    L = len(filter_bank(wave_type)[2])
    B, Cc, H, W = (int(v) for v in x_shape)
    h, w = int(shape[-2]), int(shape[-1])
    n_t, n_x = int(ori_shape[-2]), int(ori_shape[-1])
    if Cc < 8:
        raise ValueError(f'burgers reconstruction: {Cc} channels; the coefficient channels 0-7 are needed')
    if not (0 < h <= H and 0 < w <= W and 2 * h >= L and 2 * w >= L):
        raise ValueError(f'burgers reconstruction: coefficient block {h} x {w} does not fit the {H} x {W} tensor or is shorter than the filter')
    if not (2 <= n_t <= 2 * h and 1 <= n_x <= 2 * w):
        raise ValueError(f'burgers reconstruction: field {n_t} x {n_x} is not a crop of the {2 * h} x {2 * w} reconstruction')
    ss, cs, rs, es = (Cc * H * W, H * W, W, 1) if strides is None else (int(v) for v in strides)
    if B < 1 or B > 65535 or es != 1 or rs < W or cs < H * rs or ss < Cc * cs or Cc * cs >= 2 ** 31 or B * ss >= 2 ** 40:
        raise ValueError(f'burgers reconstruction: strides {(ss, cs, rs, es)} of a {tuple(x_shape)} tensor: columns must be contiguous, the '
                         'axes nested in the order sample, channel, row, and the whole inside the kernel\'s 32-bit channel offsets / grid')
    tn = min(TILE_MAX, n_t + (n_t & 1))
    while tn > 2 and lds_bytes(w, tn) > LDS_BUDGET:
        tn -= 2
    if lds_bytes(w, tn) > LDS_BUDGET:
        raise ValueError(f'burgers reconstruction: a two-row tile of a block with {w} columns needs {lds_bytes(w, tn)} B of LDS (> {LDS_BUDGET})')
    ntile = -(-n_t // tn)
    tn = -(-n_t // ntile)
    tn += tn & 1
    ntile = -(-n_t // tn)
    return dict(B=B, C=Cc, H=H, W=W, sample_stride=ss, chan_stride=cs, row_stride=rs, h=h, w=w, n_t=n_t, n_x=n_x, L=L, mode=0, tn=tn, ntile=ntile,
                lds_bytes=lds_bytes(w, tn))


_filt = {}


def _flat_rescaler(rescaler, device):
    r = torch.as_tensor(rescaler, dtype=torch.float32).reshape(-1)
    r = r.expand(8) if r.numel() == 1 else r
    if r.numel() < 8:
        raise ValueError(f'burgers reconstruction: RESCALER has {r.numel()} channels; the coefficient channels 0-7 are needed')
    return r.to(device).contiguous()


def reconstruct_generic(x, shape, ori_shape, rescaler, wave_type, pad_mode):
    """The reference's route on this tree's operators (any wavelet the DWT kernels take): rescale, tensor_to_coef, DWTInverse, crop."""
    from wdno_amd.wavelets import DWTInverse
    from wave_trans import tensor_to_coef
    n_t, n_x = int(ori_shape[-2]), int(ori_shape[-1])
    r = _flat_rescaler(rescaler, x.device)[:8].reshape(1, 8, 1, 1)
    yl, yh = tensor_to_coef(x[:, :8] * r, shape)
    u_f = DWTInverse(mode=pad_mode, wave=wave_type)((yl.contiguous(), [v.contiguous() for v in yh]))[:, :, :n_t, :n_x]
    return u_f[:, 0].contiguous(), u_f[:, 1, :n_t - 1].contiguous()


def reconstruct(x, shape, ori_shape, rescaler, wave_type='bior2.4', pad_mode='periodization'):
    """(u [B, n_t, n_x], f [B, n_t - 1, n_x]) of the sampled state x [B, C, H, W] (network units, fp32, on the GPU; any view whose columns
    are contiguous is read in place); rescaler: at least 8 values in any shape, or a scalar."""
    from wdno_amd import _lib
    from wdno_amd.filters import filter_bank
    from wdno_amd.ops import _p, _stream
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4:
        raise RuntimeError(f'burgers reconstruction: x must be a float32 [B, C, H, W] tensor on the GPU, got {x.dtype} {tuple(x.shape)} on {x.device}')
    x = x.detach()
    if (wave_type, pad_mode) not in SUPPORTED:
        return reconstruct_generic(x, shape, ori_shape, rescaler, wave_type, pad_mode)
    st = list(x.stride())
    if x.shape[0] == 1:
        st[0] = x.shape[1] * st[1]           # the stride of a one-sample axis is never walked
    try:
        pl = plan(tuple(x.shape), shape, ori_shape, wave_type, pad_mode, strides=st)
    except ValueError:
        if x.is_contiguous():
            raise
        x = x.contiguous()                   # a view the kernel cannot walk (transposed, column-strided): one copy
        pl = plan(tuple(x.shape), shape, ori_shape, wave_type, pad_mode)
    r = _flat_rescaler(rescaler, x.device)
    filt = _filt.get(wave_type)
    if filt is None:
        vals = [float(v) for bank in filter_bank(wave_type) for v in bank]
        filt = _filt[wave_type] = (C.c_float * len(vals))(*vals)
    with torch.cuda.device(x.device):
        u = torch.empty((pl['B'], pl['n_t'], pl['n_x']), dtype=torch.float32, device=x.device)
        f = torch.empty((pl['B'], pl['n_t'] - 1, pl['n_x']), dtype=torch.float32, device=x.device)
        desc = _lib.BurgersReconstructDesc(**pl)
        _lib.check(_lib.load().wdno_burgers_reconstruct(_p(x), _p(r), _p(u), _p(f), C.byref(desc), filt, _stream()), 'wdno_burgers_reconstruct')
    return u, f
