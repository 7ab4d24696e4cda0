"""The fields of a sampled smoke state on the GPU: InferencePipeline.run_base_model's wavelet branch (smoke/inference_2d.py:137-152) as one
launch of csrc/smoke_reconstruct.hip (include/wdno_hip.h: wdno_smoke_reconstruct).

The reference multiplies the sample by RESCALER, unpacks it (tensor_to_coef: a copying reshape and eight band copies), runs waverec3,
crops, reshapes, permutes, takes two means of the last channel, a 1-D IDWT, expands and concatenates. Here the coefficients are read in
place in the packed state, the product with RESCALER is formed on the fly, and pred [B, to, 6, ho, wo] is written once, in the
reference's layout.

reconstruct() -- the launch, on torch's current stream. x may be a non-contiguous view whose columns are contiguous: its strides are passed.
plan()        -- pure Python: the descriptor's integers, the tile and its LDS bytes; needs neither the library nor a GPU.

Tile rule. A workgroup owns (tn frames, hn rows, full width) of one field and runs the passes in the order T, H, W, so its two buffers are
wc (not wo) columns wide: [4][tn][hn/2 + 2][wc] after the T pass, [2][tn][hn][wc] after the H pass. The first pair of TILES whose buffers
fit 64 KiB is taken: (4, 8) at 21 760 B on the 34 x 34 block, which leaves room for seven workgroups on a compute unit's 160 KiB, and
(4, 8) at 42 240 B on the 66 x 66 block of the space super-resolution level (three workgroups).

A cascade level (InferencePipeline.run_super_model, smoke/inference_2d.py:213-231) is the same launch with the block read at offset 1
(upsample_type='space'; a view x[..., 1:, 1:] would move the smoke-out rows as well) and the smoke-out rows split at half = int(H / 2).
"""
import ctypes as C

import torch

from wdno_amd.smoke.guidance import LDS_BUDGET, SUPPORTED, _split_row

TILES = ((4, 8), (4, 4), (2, 4), (2, 2))          # (tn, hn), in order of preference
REDUCE_BYTES = 8 * 256                            # the fp64 tree of a smoke-out workgroup


def lds_bytes(wc, tn, hn):
    """LDS of a workgroup: the tile's two buffers, or the smoke-out workgroup's reduction tree and its 2 (tn/2 + 2) means."""
    return max(4 * (4 * tn * (hn // 2 + 2) * wc + 2 * tn * hn * wc), REDUCE_BYTES + 8 * (tn // 2 + 2))


def _offset(upsample_type):
    """tensor_to_coef's first row and column of the coefficient block (smoke/wave_trans_2d.py:17-33)."""
    if upsample_type is None:
        return 0
    if upsample_type == 'space':
        return 1
    raise ValueError(f'smoke reconstruction: upsample_type {upsample_type!r}; None and \'space\' are built (\'time\' has no evaluation route in the '
                     'reference\'s driver)')


def plan(x_shape, shape, ori_shape, wave_type='bior1.3', pad_mode='zero', strides=None, upsample_type=None, half=None):
    """Host integers of one wdno_smoke_reconstruct call on x of x_shape = (B, F, C, H, W) with element `strides` (default: contiguous).
    ValueError for a (wave, mode) the kernel is not built for, a block larger than the tensor, a crop larger than the reconstruction,
    strides the kernel cannot walk, and tiles that do not fit the LDS budget. upsample_type='space' (a cascade level, inference_2d.py:219):
    the block is read at rows and columns 1 .. 1 + hc, the plan gains the key `off` and the call is wdno_smoke_reconstruct_at; half: the
    split row of the smoke-out means (inference_2d.py:225-226: int(H / 2)) instead of _split_row(H). With the defaults the plan is the
    descriptor of wdno_smoke_reconstruct, key for key."""
    from wdno_amd.filters import filter_bank
    if (wave_type, pad_mode) not in SUPPORTED:
        raise ValueError(f'smoke reconstruction kernel: (wave, mode) = ({wave_type!r}, {pad_mode!r}) is not built; supported: {sorted(SUPPORTED)}')
    L = len(filter_bank(wave_type)[2])
    B, F, Cc, H, W = (int(v) for v in x_shape)
    tc, hc, wc = (int(v) for v in shape)
    to, ho, wo = (int(v) for v in ori_shape)
    if Cc < 42:
        raise ValueError(f'smoke reconstruction: {Cc} channels; 40 coefficient channels and the two condition channels are needed')
    off = _offset(upsample_type)
    if not (3 <= tc <= F and 3 <= hc <= H - off and 3 <= wc <= W - off):
        raise ValueError(f'smoke reconstruction: coefficient block {(tc, hc, wc)} at offset {off} does not fit the {(F, H, W)} tensor or is '
                         'shorter than the filter')
    half = _split_row(H) if half is None else int(half)
    if not 1 <= half < H:
        raise ValueError(f'smoke reconstruction: split row {half} leaves one of the two smoke-out means of {H} rows empty')
    rec = tuple(2 * v - L + 2 for v in (tc, hc, wc))
    if not all(1 <= o <= r for o, r in zip((to, ho, wo), rec)):
        raise ValueError(f'smoke reconstruction: field {(to, ho, wo)} is not a crop of the {rec} reconstruction')
    if B < 1 or B > 65535 or F * Cc * H * W >= 2 ** 31 or to * 6 * ho * wo >= 2 ** 31 or H < 2:
        raise ValueError(f'smoke reconstruction: tensor {tuple(x_shape)} is outside the kernel\'s 32-bit strides / grid')
    ss, fs, cs, rs, es = (F * Cc * H * W, Cc * H * W, H * W, W, 1) if strides is None else (int(v) for v in strides)
    if es != 1 or rs < W or cs < H * rs or fs < Cc * cs or ss < F * fs or B * ss >= 2 ** 40 or ss >= 2 ** 31:
        raise ValueError(f'smoke reconstruction: strides {(ss, fs, cs, rs, es)} of a {tuple(x_shape)} tensor: columns must be contiguous and '
                         'the axes nested in the order sample, frame, channel, row')
    ev = lambda v: v + (v & 1)
    tiles = [(min(tn, ev(to)), min(hn, ev(ho))) for tn, hn in TILES]
    tiles = [t for t in tiles if lds_bytes(wc, *t) <= LDS_BUDGET]
    if not tiles:
        raise ValueError(f'smoke reconstruction: the smallest tile of a block with {wc} columns does not fit {LDS_BUDGET} B of LDS')
    tn, hn = tiles[0]
    pl = dict(B=B, F=F, C=Cc, H=H, W=W, sample_stride=ss, frame_stride=fs, chan_stride=cs, row_stride=rs, tc=tc, hc=hc, wc=wc, to=to, ho=ho,
              wo=wo, L=L, mode=1, half=half, tn=tn, hn=hn, lds_bytes=lds_bytes(wc, tn, hn))
    if upsample_type is not None:
        pl['off'] = off
    return pl


_filt = {}


def level_rescaler(rescaler, channels):
    """The `channels` values a cascade level is scaled by (inference_2d.py:215, 224): entries :channels - 1 of the super model's RESCALER for the
    coefficient and condition channels and its LAST entry for the smoke-out channel -- for the 42-channel base sample entries :41 and 81."""
    r = torch.as_tensor(rescaler, dtype=torch.float32).reshape(-1)
    return torch.cat((r[:channels - 1], r[-1:]))


def reconstruct(x, shape, ori_shape, rescaler, wave_type='bior1.3', pad_mode='zero', upsample_type=None, half=None):
    """pred [B, to, 6, ho, wo] of the sampled state x [B, F, C, H, W] (network units, fp32, on the GPU); rescaler: C values in any shape.
    upsample_type, half: see plan(); the smoke-out means run over the whole rows [:half] / [half:] whatever the block's offset."""
    from wdno_amd import _lib
    from wdno_amd.filters import filter_bank
    from wdno_amd.ops import _p, _stream
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 5:
        raise RuntimeError(f'smoke reconstruction: x must be a float32 [B, F, C, H, W] tensor on the GPU, got {x.dtype} {tuple(x.shape)} on {x.device}')
    x = x.detach()
    st = list(x.stride())
    if x.shape[0] == 1:
        st[0] = x.shape[1] * st[1]           # the stride of a one-sample axis is never walked
    try:
        pl = plan(tuple(x.shape), shape, ori_shape, wave_type, pad_mode, strides=st, upsample_type=upsample_type, half=half)
    except ValueError:
        if x.is_contiguous():
            raise
        x = x.contiguous()                   # a view the kernel cannot walk (transposed, column-strided): one copy
        pl = plan(tuple(x.shape), shape, ori_shape, wave_type, pad_mode, upsample_type=upsample_type, half=half)
    r = torch.as_tensor(rescaler, dtype=torch.float32).reshape(-1).to(x.device).contiguous()
    if r.numel() != x.shape[2]:
        raise ValueError(f'smoke reconstruction: RESCALER has {r.numel()} channels, x has {x.shape[2]}')
    filt = _filt.get(wave_type)
    if filt is None:
        vals = [float(v) for bank in filter_bank(wave_type) for v in bank]
        filt = _filt[wave_type] = (C.c_float * len(vals))(*vals)
    with torch.cuda.device(x.device):
        pred = torch.empty((pl['B'], pl['to'], 6, pl['ho'], pl['wo']), dtype=torch.float32, device=x.device)
        off = pl.pop('off', None)
        desc = _lib.SmokeReconstructDesc(**pl)
        if off is None:
            _lib.check(_lib.load().wdno_smoke_reconstruct(_p(x), _p(r), _p(pred), C.byref(desc), filt, _stream()), 'wdno_smoke_reconstruct')
        else:
            _lib.check(_lib.load().wdno_smoke_reconstruct_at(_p(x), _p(r), _p(pred), C.byref(desc), off, filt, _stream()), 'wdno_smoke_reconstruct_at')
    return pred
