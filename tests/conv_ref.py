"""Convolutions (forward, data gradient, weight gradient, bias and residual gradient) in plain torch on the CPU, fp64, with the case
matrix, the input families and the two gates of tests/test_gpu_conv_matrix.py. Test infrastructure only, checked against F.conv*d and
autograd by tests/test_host_conv_ref.py.

What the split kernels compute (wdno_amd/csrc/conv_h3.hip:3-9). A tensor v with maximum amax is stored as two fp16 planes of t = v s,
s the power of two with amax s in [2^14, 2^15):  hi = fp16(t), lo = fp16(t - hi)  (planes() below is plane_pack in torch). A product is
ah bh + ah bl + al bh on exact fp16 products in fp32 accumulators, so with A = x planes, B = w planes

    y  = (conv(xh, wh + wl) + conv(xl, wh)) / (sx sw) + bias + residual
    dx = (convT(gh, wh + wl) + convT(gl, wh)) / (sg sw) + skip gradient        (the weight planes are those of the same tensor, flipped)
    dw = (corr(gh, xh + xl) + corr(gl, xh)) / (sg sx)                          db = column sums of dy, dres = dy

planes_reference() evaluates exactly that in fp64; reference() is the convolution of the fp32 values themselves.

THE EXACT GATE (families int1, int2). Inputs are chosen so that every term above, and every partial sum of them in ANY order, is an
integer multiple of one unit and smaller than 2^24 units: the kernels then have to return planes_reference() rounded once to fp32, bit
for bit -- whatever the tile shape, the split over blocks or the order of a reduction. exactness() computes sum |terms| / unit per output
element from the emulated planes; tests/test_host_conv_ref.py asserts it is below 2^24 for every (case, family, pass).
  int1  integers in [-4, 4] (amax 4, s = 2^12): lo = 0, hi exact; unit 2^24 in the accumulator, 1 after the scale.
  int2  0 or +-4096 + b, b in {-1, 0, 1}, one element planted at 4097 (s = 4): hi = +-2^14, lo = 4 b -- also at the tie 16380. The
        result is conv(x, w) - conv(bx, bw); unit 2^16 in the accumulator. Bias, residual and skip gradient are multiples of 4096 so
        that the epilogue's additions stay on the grid. Long reductions are thinned (density()) until the condition holds.

THE ELEMENT-WISE GATE (families gauss, range):  |got - ref| <= K 2^-24 scale + flush  with
    scale(y)  = conv(|x|, |w|) + |bias| + |residual| + |y|        scale(dx) = convT(|dy|, |w|) + |skip| + |dx|
    scale(dw) = corr(|dy|, |x|) + |dw|                            scale(db) = sum |dy| + |db|
    flush(y)  = 2^-40 (amax(x) sum_window |w| + amax(w) sum_window |x|)   and its analogues: lo planes below 2^-14 in scaled units are
                sub-normal fp16 and carry an absolute error of 2^-25 / s <= 2^-39 amax (conv_h3.hip:8-9).
K is NOT taken from the kernels: transcription() forms the emulated planes and sums the three plane products with torch's fp32
convolutions on the CPU. Its worst ratio over the matrix, per output kind and per reduction-length class (short: R < 2048 terms, long:
the rest), is re-measured by tests/test_host_conv_ref.py and held to K / 2:

    MEASURED = {('y', 'short'): 4.98, ('y', 'long'): 4.57, ('dx', 'short'): 4.89, ('dx', 'long'): 6.09,
                ('dw', 'short'): 5.68, ('dw', 'long'): 5.58, ('db', 'short'): 0.38, ('db', 'long'): 0.15}

(Most of that is not summation order: the dropped al bl product and the rounding of lo are up to 2^-22 of every product, four units of the
gate, and the transcription carries them like the kernels do.)
K = ceil(4 x measured): the order of an fp32 sum moves its rounding error by a small factor, the rounding inside one matrix
instruction's 16-term step is not ours to specify, and the split runs add one more level.
"""
import collections
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests.helpers import _hash_values

U = 2.0 ** -24
LONG = 2048          # reduction lengths from here on are gated with the 'long' K

K = {('y', 'short'): 20, ('y', 'long'): 19, ('dx', 'short'): 20, ('dx', 'long'): 25,
     ('dw', 'short'): 23, ('dw', 'long'): 23, ('db', 'short'): 2, ('db', 'long'): 1}

# ----------------------------------------------------------------------------------------------------------- the matrix
# xs = (N, C, *spatial), ws = (K, C, *taps) in the reference layout. mode: library debug mode the case runs under (0 = production).
# zbox: (channels, d0, h0, w0) of a zero box stated about x (ops.set_zero_box; the inputs are zero there).
# plan: what the library must choose for the forward, the data gradient and the weight gradient (plan strings of fwd_plan_str /
# wgrad_plan_str; None = that pass does not run on a split kernel; checked on the CPU by tests/test_host_conv_ref.py, and again on the device).
Case = collections.namedtuple('Case', 'name xs ws stride padding bias residual skip mode plan range zbox')


def _c(name, xs, ws, stride=1, padding=1, bias=True, residual=False, skip=False, mode=0, plan=None, rng=False, zbox=None):
    return Case(name, xs, ws, stride, padding, bias, residual, skip, mode, plan, rng, zbox)


CASES = [
    # exact fp32 (below H3_MIN_PIXELS / H3_MIN_REDUCTION)
    _c('fp32_few_pixels', (2, 64, 5, 9, 7), (64, 64, 3, 3, 3), rng=True,
       plan=(None, None, None)),      # 630 pixels
    _c('fp32_short_reduction', (2, 4, 4, 16, 16), (4, 4, 1, 3, 3), padding=(0, 1, 1), residual=True,
       plan=(None, None, None)),      # 36 terms
    # register-staged forward / data gradient (natural below 64 tiles of 64 x 64; mode 5 beyond) and weight gradient (mode 5)
    _c('reg_128x128', (17, 32, 8, 8), (136, 32, 3, 3), mode=5, rng=True,
       plan=('h3:128x128 t18 g18', 'h3:64x64 t17 g17', 'h3:128x192 s3 p384')),      # 1088 pixels: 17 < 2 x 9 row tiles
    _c('reg_64x128', (4, 8, 40, 40), (136, 8, 3, 3), mode=5,
       plan=('h3:64x128 t200 g200', 'h3:64x64 t100 g100', 'h3:128x192 s13 p512')),      # 100 x 2 tiles of 64 x 128
    _c('reg_64x64', (4, 64, 16, 16), (72, 64, 3, 3), mode=5, skip=True,
       plan=('h3:64x64 t32 g32', 'h3:64x64 t16 g16', 'h3:128x192 s2 p512 tiled')),      # 18 steps: no ksplit
    _c('reg_64x64_ksplit2', (4, 256, 16, 16), (72, 256, 3, 3), residual=True,
       plan=('h3:64x64k2 t32 g32', 'h3:64x64 t64 g64', 'h3w:64x192 s2 p512 tiled')),      # 72 steps, 32 tiles of 64 x 64
    _c('reg_128x64', (1, 8, 256, 256), (16, 8, 3, 3), mode=5,
       plan=('h3:128x64 t512 g512', 'h3:128x64 t512 g512', 'h3:64x128 s128 p512')),      # 512 tiles of 128 x 64
    _c('reg_narrow', (1, 36, 5, 16, 16), (20, 36, 3, 3, 3), mode=5, residual=True,
       plan=('h3:64x64 t20 g20', 'h3:64x64 t20 g20', 'h3:64x128 s3 p448')),      # C, K no multiples of 8
    _c('reg_wgrad_64x192', (6, 64, 14, 14), (64, 64, 3, 3), mode=5,
       plan=('h3:64x64 t19 g19', 'h3:64x64 t19 g19', 'h3:64x192 s3 p416')),      # kw C = 192
    # chunked DMA (mode 8 on tap geometries, natural otherwise); u: C % 32 == 0, l: C % 32 != 0. Tile shapes by cost on 256 CUs
    _c('chunk_128x128_u', (16, 32, 40, 40), (128, 32, 1, 3), padding=(0, 1), mode=8,
       plan=('h3d:128x128u t200 g200', 'h3d:192x64u t134 g134', 'h3d:128x128 s50 p512')),      # 200 tiles, one round; 192 x 64 would need two
    _c('chunk_128x128_l', (16, 16, 40, 40), (128, 16, 3, 3),
       plan=('h3d:128x128l t200 g200', 'h3t:128x64 t200 g200', 'h3d:128x128 s50 p512')),
    _c('chunk_192x128_u', (24, 32, 40, 40), (96, 32, 1, 3), padding=(0, 1), mode=8,
       plan=('h3d:192x128u t200 g200', 'h3d:192x64u t200 g200', 'h3d:128x128 s75 p512')),      # 300 tiles of 128 x 128 -> 200 of 192 x 128
    _c('chunk_192x128_l', (24, 16, 40, 40), (96, 16, 3, 3), bias=False,
       plan=('h3d:192x128l t200 g200', 'h3t:192x64 t200 g200', 'h3d:128x128 s75 p512')),
    _c('chunk_256x64_u', (36, 32, 40, 40), (32, 32, 1, 3), padding=(0, 1), mode=8,
       plan=('h3d:256x64u t225 g225', 'h3d:256x64u t225 g225', 'h3d:64x128 s113 p512')),      # 225 tiles of 256 x 64; 300 of 192 x 64
    _c('chunk_256x64_l', (36, 16, 40, 40), (24, 16, 3, 3), residual=True,
       plan=('h3d:256x64l t225 g225', 'h3d:256x64l t225 g225', 'h3d:64x128 s113 p512')),
    _c('chunk_192x64_u', (3, 32, 23, 17), (40, 32, 3, 3), mode=8, rng=True,
       plan=('h3d:192x64u t7 g7', 'h3d:192x64l t7 g7', 'h3d:64x128 s3 p416')),      # 1173 pixels: ragged last tile, ragged K
    _c('chunk_192x64_l', (3, 40, 23, 17), (72, 40, 3, 3), mode=7,
       plan=('h3d:192x64l t14 g14', 'h3d:192x64l t7 g7', 'h3d:128x128 s3 p416')),
    _c('chunk_1x1', (2, 64, 24, 40, 40), (64, 64, 1, 1, 1), padding=0,
       plan=('h3d:192x64u t400 g256', 'h3d:192x64u t400 g256', 'h3d:64x128 s150 p512')),      # one step per tile, several tiles per block
    _c('chunk_stride2', (2, 64, 4, 32, 32), (64, 64, 1, 4, 4), stride=(1, 2, 2), padding=(0, 1, 1), mode=7,
       plan=('h3d:192x64u t11 g11', 'h3d:192x64u t11 g11', 'h3d:64x128 s4 p512')),      # data gradient: four parity launches
    # tap-resident, shapes picked by cost
    _c('tap_64x64', (4, 32, 32, 32), (64, 32, 3, 3), rng=True,
       plan=('h3t:64x64 t64 g64', 'h3t:64x64 t64 g64', 'h3d:64x128 s8 p512')),      # 64 tiles
    _c('tap_128x64', (13, 32, 40, 40), (64, 32, 3, 3), skip=True,
       plan=('h3t:128x64 t163 g163', 'h3t:128x64 t163 g163', 'h3d:64x128 s41 p512')),      # 325 tiles of 64 x 64 -> 163 of 128 x 64
    _c('tap_192x64', (24, 32, 40, 40), (32, 32, 1, 3), padding=(0, 1),
       plan=('h3t:192x64 t200 g200', 'h3t:192x64 t200 g200', 'h3d:64x128 s75 p512')),      # 200 tiles
    _c('tap_256x64', (36, 32, 40, 40), (32, 32, 1, 3), padding=(0, 1),
       plan=('h3t:256x64 t225 g225', 'h3t:256x64 t225 g225', 'h3d:64x128 s113 p512')),      # 225 tiles
    _c('tap_128x128', (16, 32, 40, 40), (128, 32, 1, 3), padding=(0, 1), residual=True,
       plan=('h3t:128x128 t200 g200', 'h3t:128x64 t200 g200', 'h3d:128x128 s50 p512')),
    _c('tap_192x128', (28, 32, 40, 40), (96, 32, 1, 3), padding=(0, 1),
       plan=('h3t:192x128 t234 g234', 'h3t:192x64 t234 g234', 'h3d:128x128 s88 p512')),      # 234 tiles
    _c('tap_320x64_rounds', (2, 32, 24, 40, 40), (32, 32, 3, 1, 3), padding=(1, 0, 1),
       plan=('h3t:320x64 t240 g240', 'h3t:320x64 t240 g240', 'h3d:64x128 s150 p512')),      # 240 tiles of 320 x 64 instead of 300 / 400
    _c('tap_several_rounds', (4, 32, 24, 40, 40), (32, 32, 3, 1, 3), padding=(1, 0, 1),
       plan=('h3t:320x64 t480 g256', 'h3t:320x64 t480 g256', 'h3d:64x128 s166 p928')),      # more tiles than blocks, ragged last round
    # five-row tiles forced on small cases; rows of 5 and 7 pixels: tiles cross rows, planes and samples
    _c('tap_160x128_forced', (3, 32, 7, 10, 5), (96, 32, 3, 3, 3), mode=30,
       plan=('h3t:160x128 t7 g7', 'h3t:320x64 t4 g4', 'h3d:128x128 s3 p352')),
    _c('tap_320x64_forced', (3, 32, 7, 7, 7), (64, 32, 3, 3, 3), mode=31,
       plan=('h3t:320x64 t4 g4', 'h3t:320x64 t4 g4', 'h3d:64x128 s3 p352')),
    # the four-run split, with and without residual, refused by mode 56
    _c('split4', (17, 512, 8, 8), (520, 512, 3, 3),
       plan=('h3t:128x128/4 t45 g180', 'h3:128x128 t36 g36', 'h3w:64x192 s2 p544 pair tiled')),      # ragged K, half a pixel tile at the end
    _c('split4_residual', (4, 256, 4, 8, 8), (256, 256, 3, 3, 3), residual=True, bias=False,
       plan=('h3t:128x128/4 t16 g64', 'h3t:128x128/4 t16 g64', 'h3w:64x192 s2 p512 tiled')),
    _c('split4_mode56', (4, 256, 4, 8, 8), (256, 256, 3, 3, 3), mode=56,
       plan=('h3t:64x64 t64 g64', 'h3t:64x64 t64 g64', 'h3w:64x192 s2 p512 tiled')),
    # geometry edges of the tap-resident kernels (mode 7: below 64 tiles of 64 x 64)
    _c('tap_w2', (8, 32, 4, 16, 2), (32, 32, 3, 3, 3), mode=7,
       plan=('h3t:64x64 t16 g16', 'h3t:64x64 t16 g16', 'h3d:64x128 s2 p512 tiled')),      # both W neighbours missing somewhere in every row
    _c('tap_133', (2, 64, 6, 12, 12), (128, 64, 1, 3, 3), padding=(0, 1, 1), mode=7,
       plan=('h3t:64x64 t54 g54', 'h3t:64x64 t27 g27', 'h3w:64x192 s4 p448')),
    _c('tap_313', (2, 64, 6, 12, 12), (64, 64, 3, 1, 3), padding=(1, 0, 1), mode=7,
       plan=('h3t:64x64 t27 g27', 'h3t:64x64 t27 g27', 'h3w:64x192 s4 p448')),
    _c('tap_ragged_k40', (3, 128, 4, 10, 10), (40, 128, 3, 3, 3), mode=7,
       plan=('h3t:64x64 t19 g19', 'h3d:192x64l t14 g14', 'h3w:64x192 s3 p416')),      # two channel tiles in the weight gradient
    # window weight gradient: split pairs (odd split count), mode 70, K > 64 under mode 11, two channel tiles x two k tiles
    _c('wgrad_pair_odd', (17, 256, 16, 16), (256, 256, 3, 3),
       plan=('h3t:128x64 t136 g136', 'h3t:128x64 t136 g136', 'h3w:64x192 s9 p512 pair')),      # 9 splits: the last pair holds one window; 4 x 4 tiles
    _c('wgrad_mode70', (17, 256, 16, 16), (256, 256, 3, 3), mode=70,
       plan=('h3t:128x64 t136 g136', 'h3t:128x64 t136 g136', 'h3w:64x192 s8 p544 tiled')),
    _c('wgrad_mode11', (3, 64, 17, 21), (72, 64, 3, 3), mode=11,
       plan=('h3:128x128 t9 g9', 'h3:64x64 t17 g17', 'h3d:128x192 s3 p384')),
    _c('wgrad_2x2_tiles', (5, 128, 16, 16), (128, 128, 3, 3), rng=True,
       plan=('h3:64x64 t40 g40', 'h3:64x64 t40 g40', 'h3w:64x192 s3 p448')),
    _c('wgrad_mode6', (2, 32, 24, 40, 40), (32, 32, 1, 1, 3), padding=(0, 0, 1), mode=6,
       plan=('h3t:320x64 t240 g240', 'h3t:320x64 t240 g240', 'h3d:64x128 s150 p512')),
    # the 7-wide stem (mode 7 near the 1024-pixel threshold; natural from 100 tiles of 256 pixels on)
    _c('stem_192', (1, 42, 4, 16, 17), (16, 42, 7, 7, 7), padding=3, mode=7, zbox=(32, 3, 12, 17), rng=True,
       plan=('h3t_stem:192x64 t6 g6', 'h3t_stem:192x64 t6 g6', 'h3s:64x352 s3 p384')),      # 1088 pixels: 5 tiles of 256, 6 of 192
    _c('stem_2d_k40', (2, 42, 31, 19), (40, 42, 7, 7), padding=3, mode=7,
       plan=('h3t_stem:192x64 t7 g7', 'h3d:192x64l t7 g7', 'h3s:64x352 s3 p416')),      # ragged K; the data gradient has 40 channels: chunked
    _c('stem_2d_natural', (16, 42, 40, 40), (8, 42, 7, 7), padding=3,
       plan=('h3t_stem:192x64 t134 g134', 'h3d:192x64l t134 g134', 'h3s:64x352 s35 p736')),      # 100 tiles of 256 -> 134 of 192
    _c('stem_2d_mode72', (16, 42, 40, 40), (8, 42, 7, 7), padding=3, mode=72,
       plan=('h3t_stem:256x64 t100 g100', 'h3d:192x64l t134 g134', 'h3s:64x352 s35 p736')),
    # more stem tiles than blocks (256-pixel tiles then), with a zero box, and the same with the hint ignored (mode 57)
    _c('stem_several_rounds', (1, 42, 11, 80, 80), (8, 42, 3, 3, 7), padding=(1, 1, 3), zbox=(32, 8, 60, 80),
       plan=('h3t_stem:256x64 t275 g256', 'h3d:192x64l t367 g256', 'h3s:64x352 s28 p2528')),
    _c('stem_mode57', (1, 42, 11, 80, 80), (8, 42, 3, 3, 7), padding=(1, 1, 3), zbox=(32, 8, 60, 80), mode=57,
       plan=('h3t_stem:256x64 t275 g256', 'h3d:192x64l t367 g256', 'h3s:64x352 s28 p2528')),
    # the folded 2x2 / stride-2 patch convolution and its q{py}{px} data gradient
    _c('patch2', (6, 40, 1, 36, 20), (72, 40, 1, 2, 2), stride=(1, 2, 2), padding=0,
       plan=('h3:128x128 t9 g9', 'h3:64x64 t17 g17', 'h3d:128x128 s3 p384')),
]
# Single bf16 planes (ops._math('bf16')): (case, the plans of the single-plane kernels). The wide case exists only here: the 256 x 128
# tap-resident tiles need two rounds of them.
BF16_CASES = [
    (_c('bf16_wide_256x128', (32, 32, 64, 64), (128, 32, 1, 3), padding=(0, 1)),
     ('h3t:256x128 t512 g256', 'h3t:256x64 t512 g256', 'h3d:128x128 s256 p512')),
    ('stem_192', ('h3t_stem:256x64 t5 g5', 'h3t_stem:256x64 t5 g5', 'h3s:64x352 s3 p384')),
    ('chunk_192x64_l', ('h3d:192x64l t14 g14', 'h3d:192x64l t7 g7', 'h3d:128x128 s3 p416')),
    ('wgrad_2x2_tiles', ('h3:64x64 t40 g40', 'h3:64x64 t40 g40', 'h3w:64x192 s3 p448')),
    ('tap_64x64', ('h3t:64x64 t64 g64', 'h3t:64x64 t64 g64', 'h3d:64x128 s8 p512')),
    ('reg_narrow', ('h3:64x64 t20 g20', 'h3:64x64 t20 g20', 'h3:64x128 s3 p448')),
]
BY_NAME = {c.name: c for c in CASES}
BF16_CASES = [(BY_NAME[c] if isinstance(c, str) else c, pl) for c, pl in BF16_CASES]
# the single-plane gate: |got - ref| <= K16 2^-9 scale, 2^-9 the unit roundoff of a bf16 operand; K16 = ceil(4 x the worst ratio of
# transcription(single=True) over BF16_CASES), measured {y: 0.97, dx: 0.50, dw: 0.61}; db is a sum of the fp32 dy and keeps the fp32 gate
U16 = 2.0 ** -9
K16 = {'y': 4, 'dx': 2, 'dw': 3}
FAMILIES = ('int1', 'int2', 'gauss', 'range')


def families(case):
    return ('int1', 'int2', 'gauss') + (('range',) if case.range else ())


# ----------------------------------------------------------------------------------------------------------- geometry
def _trip(v, nd, fill):
    v = (v,) * nd if isinstance(v, int) else tuple(v)
    return (fill,) * (3 - nd) + v


def dims(case):
    """n, c, k, sp (D, H, W), ks, st, pd, osp of a case, 3-D throughout."""
    nd = len(case.ws) - 2
    n, c = case.xs[:2]
    sp = (1,) * (3 - nd) + tuple(case.xs[2:])
    ks = (1,) * (3 - nd) + tuple(case.ws[2:])
    st, pd = _trip(case.stride, nd, 1), _trip(case.padding, nd, 0)
    osp = tuple((a + 2 * p - kk) // s + 1 for a, kk, s, p in zip(sp, ks, st, pd))
    return n, c, case.ws[0], sp, ks, st, pd, osp


def reduction_lengths(case):
    """Terms per output element of the three passes: C taps, K taps, output pixels."""
    n, c, k, sp, ks, st, pd, osp = dims(case)
    taps = ks[0] * ks[1] * ks[2]
    return {'y': c * taps, 'dx': k * taps, 'dw': n * osp[0] * osp[1] * osp[2], 'db': n * osp[0] * osp[1] * osp[2]}


def k_of(case, name):
    kind = {'y': 'y', 'dx': 'dx', 'dw': 'dw', 'db': 'db'}[name]
    return K[(kind, 'long' if reduction_lengths(case)[name] >= LONG else 'short')]


FWD_FAMILY = ('fp32', 'h3', 'h3d', 'h3t', 'h3t_stem')
WGRAD_FAMILY = ('h3', 'h3d', 'h3w', 'h3s')


def fwd_plan_str(pl):
    fam = FWD_FAMILY[pl.family]
    s = f'{fam}:{pl.bm}x{pl.bn}'
    if pl.tsplit > 1:
        s += f'/{pl.tsplit}'
    if pl.ksplit > 1:
        s += f'k{pl.ksplit}'
    if fam == 'h3d':
        s += 'u' if pl.uniform else 'l'
    return s + f' t{pl.ntiles} g{pl.grid}'


def wgrad_plan_str(pl):
    return (f'{WGRAD_FAMILY[pl.family]}:{pl.bm}x{pl.bn} s{pl.splits} p{pl.pix_per_split}' + (' pair' if pl.splitpair else '') +
            (' tiled' if pl.reduce_tiled else ''))


def launches(ops, case, lowp=False):
    """The split-kernel launches conv_cl and its backward make for a case, as (pass, kind, geometry, extra): the geometry arithmetic of
    wdno_amd/ops.py::_Conv (channel padding to 4 in tensors, to 8 -- whole 16-channel blocks for a stem -- in planes). The device test holds
    this list against ops.LAUNCH_LOG, so that the plans asserted on the CPU are the plans of the launches that really happen.
    pass: 'y', 'dx' (one entry per launch) or 'dw'; None where that pass does not run on a split kernel."""
    n, c, k, sp, ks, st, pd, osp = dims(case)
    cp, kp = ops.pad4(c), ops.pad4(k)
    taps = ks[0] * ks[1] * ks[2]
    pix_out, pix_in = n * osp[0] * osp[1] * osp[2], n * sp[0] * sp[1] * sp[2]
    out = []
    h3 = ops._use_h3(pix_out, cp * taps)
    c8 = ops.pad8(cp)
    if ks[2] == 7 and kp <= 64 and st == (1, 1, 1) and c8 % 16:
        c8 += 8
    if h3:
        out.append(('y', 'fwd', ops._geom((n, *sp), c8, kp, ks, st, pd, osp), (lowp, case.residual)))
    k8 = ops.pad8(kp)
    if st == (1, 1, 1) and ops._use_h3(pix_in, kp * taps):          # (whatever the forward ran on)
        gd = ops._geom((n, *osp), k8, cp, ks, (1, 1, 1), tuple(kk - 1 - p for kk, p in zip(ks, pd)), sp)
        out.append(('dx', 'fwd', gd, (lowp, case.skip)))
    elif not h3:
        pass
    elif ks == (1, 2, 2) and st == (1, 2, 2) and pd == (0, 0, 0) and ops._use_h3(pix_out, kp) and ops.PATCH_DGRAD_H3:
        for py in range(2):
            for px in range(2):
                gd = ops._geom((n, *osp), k8, cp, (1, 1, 1), (1, 1, 1), (0, 0, 0), osp, y_sp=sp, ostride=(1, 2, 2), ooff=(0, py, px))
                out.append(('dx', 'fwd', gd, (lowp, False)))
    elif ks == (1, 4, 4) and st == (1, 2, 2) and pd == (0, 1, 1) and ops._use_h3(pix_out, kp * 4):
        for py in range(2):
            for px in range(2):
                gd = ops._geom((n, *osp), k8, cp, (1, 2, 2), (1, 1, 1), (0, 1 - py, 1 - px), osp, y_sp=sp, ostride=(1, 2, 2), ooff=(0, py, px))
                out.append(('dx', 'fwd', gd, (lowp, False)))            # parity classes of ops.conv_transpose_h3
    if h3:
        out.append(('dw', 'wgrad', ops._geom((n, *sp), c8, k8, ks, st, pd, osp), (lowp, (k, c))))
    return out


def lent_ws(ops, g, lowp):
    """Bytes of split workspace the plan of a forward launch is asked about: what the library wants for the geometry, since
    ops.conv_fwd_h3 lends exactly that (the device test holds this against the wsb the launch logged)."""
    import ctypes as C
    return 0 if lowp else int(ops._lib_().wdno_conv_fwd_split_ws_bytes(C.byref(g)))


def plan_of(ops, kind, g, extra):
    """Plan string of one launch, from the library. (The residual of ops.conv_cl is never y itself.)"""
    if kind == 'fwd':
        lowp, has_res = extra
        return fwd_plan_str(ops.conv_fwd_plan(g, lowp, False, lent_ws(ops, g, lowp)))
    lowp, (kn, cn) = extra
    return wgrad_plan_str(ops.conv_wgrad_plan(g, lowp, kn, cn))


def plans(ops, case, lowp=False):
    """(forward, data gradient, weight gradient) plan strings of a case under the CURRENT debug mode; None = no split kernel. The data
    gradient's launches (four for the patch convolution) must agree among themselves."""
    res = {'y': None, 'dx': None, 'dw': None}
    for name, kind, g, extra in launches(ops, case, lowp):
        s = plan_of(ops, kind, g, extra)
        assert res[name] in (None, s), (case.name, name, res[name], s)
        res[name] = s
    return res['y'], res['dx'], res['dw']


# ----------------------------------------------------------------------------------------------------------- inputs
def _hash(shape, seed):
    return torch.from_numpy(_hash_values(int(np.prod(shape)), seed).reshape(shape))          # fp64 in [-0.5, 0.5)


def _gauss(shape, seed):
    """N(0, 1) from the integer hash (Box-Muller on two hashed uniforms; fp64, then rounded to fp32 by the caller)."""
    u1 = _hash(shape, seed) + 0.5
    u2 = _hash(shape, seed + 7919)
    return torch.sqrt(-2.0 * torch.log(u1.clamp_min(2.0 ** -33))) * torch.cos(2.0 * math.pi * u2)


def _ints(shape, seed):
    return torch.floor(_hash(shape, seed) * 9.0 + 4.5) - 4.0                                 # integers in [-4, 4]


def density(case):
    """Fractions of non-zero values of x, w and dy in family int2, thinned until sum |terms| stays below 2^24 units: the forward has
    C taps dx dw terms of 2^12 units, the data gradient K taps dg dw, the weight gradient P dx dg, and the bias gradient P dg of 1 unit
    (4096 each, unit 1)."""
    r = reduction_lengths(case)
    budget = 2800.0                                    # of the 4096 the condition allows: the thinning is random, elements differ
    dg = min(1.0, budget / r['dw'])
    dx = min(1.0, budget / (r['dw'] * dg))
    dw = min(1.0, budget / max(r['y'] * dx, r['dx'] * dg))
    return dx, dw, dg


def _int2(shape, seed, dens, plant=True):
    h = _hash(shape, seed)
    sign = torch.where(_hash(shape, seed + 1) < 0, -1.0, 1.0).double()
    b = torch.floor(_hash(shape, seed + 2) * 3.0 + 1.5) - 1.0
    v = torch.where(h + 0.5 < dens, sign * 4096.0 + b, torch.zeros_like(h))
    if plant:
        v.reshape(-1)[int((seed * 2654435761) % v.numel())] = 4097.0
    return v


def data_key(case):
    """What the data of a case depends on: cases that differ in the debug mode only share inputs and references."""
    return Case('', case.xs, case.ws, case.stride, case.padding, case.bias, case.residual, case.skip, 0, None, False, case.zbox)


def inputs(case, family):
    """fp32 CPU tensors of a case in the reference layout: x [N, C, *sp], w, bias [K] | None, res (y's shape) | None, skip (x's shape) | None,
    dy. Shared and read-only."""
    return _inputs(data_key(case), family)


@functools.lru_cache(maxsize=6)
def _inputs(case, family):
    n, c, k, sp, ks, st, pd, osp = dims(case)
    seed = (sum(case.xs) * 31 + sum(case.ws) * 17 + len(case.xs)) * 16 + FAMILIES.index(family) * 4096
    nd = len(case.ws) - 2
    ys = (n, k, *osp[3 - nd:])
    fan_in = c * ks[0] * ks[1] * ks[2]
    if family == 'int1':
        t = dict(x=_ints(case.xs, seed), w=_ints(case.ws, seed + 1), bias=_ints((k,), seed + 2), res=_ints(ys, seed + 3), dy=_ints(ys, seed + 4),
                 skip=_ints(case.xs, seed + 5))
        for key in ('x', 'w', 'dy'):
            t[key].reshape(-1)[seed % t[key].numel()] = 4.0
    elif family == 'int2':
        dx_, dw_, dg_ = density(case)
        t = dict(x=_int2(case.xs, seed, dx_), w=_int2(case.ws, seed + 10, dw_), dy=_int2(ys, seed + 40, dg_), bias=4096.0 * _ints((k,), seed + 20),
                 res=4096.0 * _ints(ys, seed + 30), skip=4096.0 * _ints(case.xs, seed + 50))
    else:
        t = dict(x=_gauss(case.xs, seed), w=_gauss(case.ws, seed + 1) / math.sqrt(fan_in), bias=_gauss((k,), seed + 2), res=_gauss(ys, seed + 3),
                 dy=_gauss(ys, seed + 4), skip=_gauss(case.xs, seed + 5))
        if family == 'range':                          # channels scaled by 2^0 .. 2^-12: the scale is per tensor, small channels live in the low bits
            fx = (2.0 ** -(torch.arange(c) % 13).double()).reshape(1, c, *([1] * nd))
            fk = (2.0 ** -(torch.arange(k) % 13).double()).reshape(1, k, *([1] * nd))
            t['x'], t['skip'] = t['x'] * fx, t['skip'] * fx
            t['dy'], t['res'] = t['dy'] * fk, t['res'] * fk
    if case.zbox is not None:                          # x is zero in the first zc channels wherever d >= d0 or h >= h0 or w >= w0
        zc, d0, h0, w0 = case.zbox
        x5 = t['x'].reshape(n, c, *sp)
        x5[:, :zc, d0:], x5[:, :zc, :, h0:], x5[:, :zc, :, :, w0:] = 0.0, 0.0, 0.0
    if not case.bias:
        t['bias'] = None
    if not case.residual:
        t['res'] = None
    if not case.skip:
        t['skip'] = None
    return {key: (None if v is None else v.float()) for key, v in t.items()}


# ----------------------------------------------------------------------------------------------------------- planes
def planes(v):
    """plane_pack (csrc/common.h) in torch: (hi, lo, s) of an fp32 tensor, hi and lo as fp64 tensors holding fp16 values."""
    amax = float(v.abs().max())
    s = 2.0 ** (14 - math.frexp(amax)[1] + 1) if amax > 0 else 1.0          # amax s in [2^14, 2^15)
    t = v.double() * s
    hi = t.to(torch.float16)
    lo = (t.float() - hi.float()).to(torch.float16)
    return hi.double(), lo.double(), s


def _conv(x, w, case):
    nd = len(case.ws) - 2
    return (F.conv3d, F.conv2d)[3 - nd](x, w, None, stride=case.stride, padding=case.padding)


def _bilinear(x, w, dy, case):
    """conv(x, w), and the gradients of <conv(x, w), dy> with respect to x and w, in the dtype of the arguments."""
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = _conv(xr, wr, case)
    gx, gw = torch.autograd.grad(y, (xr, wr), dy)
    return y.detach(), gx, gw


def _finish(t, y, gx, gw, dt=torch.float64):
    dy = t['dy'].to(dt)
    out = {'y': y, 'dx': gx, 'dw': gw}
    if t['bias'] is not None:
        out['y'] = out['y'] + t['bias'].to(dt).reshape(1, -1, *([1] * (y.dim() - 2)))
        out['db'] = dy.sum(dim=[0] + list(range(2, y.dim())))
    if t['res'] is not None:
        out['y'] = out['y'] + t['res'].to(dt)
        out['dres'] = dy.clone()
    if t['skip'] is not None:
        out['dx'] = out['dx'] + t['skip'].to(dt)
    return out


def reference(t, case):
    """fp64 y, dx, dw (+ db, dres) of the fp32 values themselves: F.conv*d and autograd."""
    return _finish(t, *_bilinear(t['x'].double(), t['w'].double(), t['dy'].double(), case))


def planes_reference(t, case, single=False):
    """What the split kernels compute, in exact arithmetic (module docstring). single: one bf16 plane per operand, one product."""
    if single:
        q = lambda v: v.to(torch.bfloat16).double()
        return _finish(t, *_bilinear(q(t['x']), q(t['w']), q(t['dy']), case))
    (xh, xl, sx), (wh, wl, sw), (gh, gl, sg) = planes(t['x']), planes(t['w']), planes(t['dy'])
    y = (_conv(xh, wh + wl, case) + _conv(xl, wh, case)) / (sx * sw)
    _, gx1, _ = _bilinear(xh, wh + wl, gh, case)
    _, gx2, _ = _bilinear(xh, wh, gl, case)
    _, _, gw1 = _bilinear(xh + xl, wh, gh, case)
    _, _, gw2 = _bilinear(xh, wh, gl, case)
    return _finish(t, y, (gx1 + gx2) / (sg * sw), (gw1 + gw2) / (sg * sx))


def transcription(t, case, single=False):
    """The kernels' arithmetic in fp32 torch on the CPU: the emulated planes, the three plane products summed by torch's fp32
    convolutions, the scale, bias, residual and skip gradient in fp32."""
    f32 = torch.float32
    if single:
        q = lambda v: v.to(torch.bfloat16).to(f32)
        y, gx, gw = _bilinear(q(t['x']), q(t['w']), q(t['dy']), case)
        return _finish(t, y, gx, gw, f32)
    (xh, xl, sx), (wh, wl, sw), (gh, gl, sg) = [tuple(p.to(f32) if torch.is_tensor(p) else p for p in planes(t[key])) for key in ('x', 'w', 'dy')]
    y = ((_conv(xh, wh, case) + _conv(xh, wl, case)) + _conv(xl, wh, case)) * f32_scalar(1.0 / (sx * sw))
    gx = sum_f32(_bilinear(xh, wh, gh, case)[1], _bilinear(xh, wl, gh, case)[1], _bilinear(xh, wh, gl, case)[1]) * f32_scalar(1.0 / (sg * sw))
    gw = sum_f32(_bilinear(xh, wh, gh, case)[2], _bilinear(xl, wh, gh, case)[2], _bilinear(xh, wh, gl, case)[2]) * f32_scalar(1.0 / (sg * sx))
    return _finish(t, y, gx, gw, f32)


def f32_scalar(v):
    return torch.tensor(v, dtype=torch.float32)


def sum_f32(a, b, c):
    return (a + b) + c


def scales(t, case, ref):
    """({name: scale}, {name: flush}) of the element-wise gate (module docstring), fp64."""
    xa, wa, ga = t['x'].double().abs(), t['w'].double().abs(), t['dy'].double().abs()
    y, gx, gw = _bilinear(xa, wa, ga, case)
    ones_x, ones_w, ones_g = torch.ones_like(xa), torch.ones_like(wa), torch.ones_like(ga)
    ax, aw, ag = float(xa.max()), float(wa.max()), float(ga.max())
    yx, gxg, gwg = _bilinear(xa, ones_w, ga, case)            # sums of |x| over a window; of |dy| over its reach; of |dy| over the pixels of a tap
    y1, gx1, gw1 = _bilinear(ones_x, wa, ones_g, case)        # sums of |w| over a window (padding left out) ...
    _, _, gwx = _bilinear(xa, ones_w, ones_g, case)           # ... and of |x| over the pixels of a tap
    fl = {'y': 2.0 ** -40 * (ax * y1 + aw * yx), 'dx': 2.0 ** -40 * (ag * gx1 + aw * gxg), 'dw': 2.0 ** -40 * (ag * gwx + ax * gwg)}
    sc = {'y': y, 'dx': gx, 'dw': gw}
    if t['bias'] is not None:
        sc['y'] = sc['y'] + t['bias'].double().abs().reshape(1, -1, *([1] * (y.dim() - 2)))
        sc['db'] = ga.sum(dim=[0] + list(range(2, y.dim())))
        fl['db'] = torch.zeros_like(sc['db'])
    if t['res'] is not None:
        sc['y'] = sc['y'] + t['res'].double().abs()
    if t['skip'] is not None:
        sc['dx'] = sc['dx'] + t['skip'].double().abs()
    return {k: v + ref[k].abs() for k, v in sc.items()}, fl


def exactness(t, case, family):
    """{name: max over elements of sum |terms| / unit} of the exact gate, from the emulated planes; and whether hi + lo reconstructs v s
    exactly for x, w and dy. The gate is valid where every value is below 2^24."""
    (xh, xl, sx), (wh, wl, sw), (gh, gl, sg) = planes(t['x']), planes(t['w']), planes(t['dy'])
    rec = all(torch.equal(h + l, t[key].double() * s) for key, (h, l, s) in (('x', (xh, xl, sx)), ('w', (wh, wl, sw)), ('dy', (gh, gl, sg))))
    a = torch.abs
    # accumulator units: int1 -- products are multiples of 2^24 (hi = 4096 k); int2 -- of 2^16 (hi hi = 2^28, hi lo = 2^16 b b')
    unit = 2.0 ** 24 if family == 'int1' else 2.0 ** 16
    y = _conv(a(xh), a(wh) + a(wl), case) + _conv(a(xl), a(wh), case)
    _, gx1, gw1 = _bilinear(a(xh), a(wh) + a(wl), a(gh), case)
    _, gx2, _ = _bilinear(a(xh), a(wh), a(gl), case)
    _, _, gw2 = _bilinear(a(xl), a(wh), a(gh), case)
    _, _, gw3 = _bilinear(a(xh), a(wh), a(gl), case)
    out = {'y': y / unit, 'dx': (gx1 + gx2) / unit, 'dw': (gw1 + gw2 + gw3) / unit}
    # after the scale the unit is unit / (s s'): 1 for int1, 2^12 for int2; bias / residual / skip join there
    post = 1.0 if family == 'int1' else 4096.0
    if t['bias'] is not None:
        out['y'] = out['y'] + a(t['bias'].double()).reshape(1, -1, *([1] * (y.dim() - 2))) / post
        out['db'] = a(t['dy'].double()).sum(dim=[0] + list(range(2, y.dim())))          # column sums: unit 1 in both families
    if t['res'] is not None:
        out['y'] = out['y'] + a(t['res'].double()) / post
    if t['skip'] is not None:
        out['dx'] = out['dx'] + a(t['skip'].double()) / post
    return {k: float(v.max()) for k, v in out.items()}, rec


def expected(case, family):
    """The reference of a (case, family), computed once and shared: for the exact families planes_reference() rounded once to fp32, for
    the others (reference(), scales, flush)."""
    return _expected(data_key(case), family)


@functools.lru_cache(maxsize=6)
def _expected(case, family):
    t = _inputs(case, family)
    if family in ('int1', 'int2'):
        return {k: v.float() for k, v in planes_reference(t, case).items()}
    ref = reference(t, case)
    return (ref,) + scales(t, case, ref)


def ratio(got, ref, scale, flush=None, unit=U):
    """max of (|got - ref| - flush) / (unit scale), unit = 2^-24 unless stated."""
    err = (got.detach().double().cpu().reshape(ref.shape) - ref).abs()
    if flush is not None:
        err = (err - flush).clamp_min(0)
    r = err / (unit * scale).clamp_min(1e-300)
    return float(r.max()) if torch.isfinite(r).all() else math.inf


def wrong_elements(got, want, name, case):
    """Where an exact gate fails: count, and the index set reduced to the coordinates a kernel bug lives in."""
    bad = (got != want).nonzero()
    if bad.numel() == 0:
        return ''
    n, c, k, sp, ks, st, pd, osp = dims(case)
    msg = [f'{name}: {bad.shape[0]} of {want.numel()} elements differ']
    cols = list(zip(*bad.tolist()))
    uniq = lambda v: sorted(set(v))
    short = lambda v: (v if len(v) <= 12 else v[:6] + ['...'] + v[-3:])
    if name in ('y', 'dx', 'dres'):                     # [N, channels, *sp]: pixel rows, tiles of 64 pixels, channels
        spx = osp if name != 'dx' else sp
        nd = len(cols) - 2
        dimsz = spx[3 - nd:]
        flat = [0] * len(cols[0])
        for i in range(len(cols[0])):
            p = cols[0][i]
            for d_ in range(nd):
                p = p * dimsz[d_] + cols[2 + d_][i]
            flat[i] = p
        msg.append(f'samples {short(uniq(cols[0]))} channels {short(uniq(cols[1]))} rows(h) {short(uniq(cols[-2]))} columns(w) {short(uniq(cols[-1]))}')
        msg.append(f'pixel tiles of 64: {short(uniq([p // 64 for p in flat]))} (of 128: {short(uniq([p // 128 for p in flat]))}, of 192: '
                   f'{short(uniq([p // 192 for p in flat]))}, of 256: {short(uniq([p // 256 for p in flat]))})')
    elif name == 'dw':                                  # [K, C, *taps]
        msg.append(f'k {short(uniq(cols[0]))} c {short(uniq(cols[1]))} taps {short(uniq(list(zip(*cols[2:]))))}')
    else:
        msg.append(f'channels {short(uniq(cols[0]))}')
    i0 = tuple(bad[0].tolist())
    msg.append(f'first: {i0} got {float(got[i0])!r} want {float(want[i0])!r}')
    return '; '.join(msg)


# ----------------------------------------------------------------------------------------------------------- ConvTranspose (1,4,4) / (1,2,2) / (0,1,1)
CONVT = dict(xs=(2, 64, 4, 16, 16), cout=64)          # 2048 input pixels, 8192 output pixels; forward 4 taps x 64, data gradient 16 taps x 64 terms


@functools.lru_cache(maxsize=2)
def convt_inputs(family):
    """x [N, Cin, D, H, W], w [Cin, Cout, 1, 4, 4], bias, dy of the transposed convolution (ops.conv_transpose_cl), families int1 / int2;
    in int2 dy is thinned so that the bias gradient, a sum over 8192 pixels, stays exact."""
    xs, cout = CONVT['xs'], CONVT['cout']
    ws, ys = (xs[1], cout, 1, 4, 4), (xs[0], cout, xs[2], 2 * xs[3], 2 * xs[4])
    if family == 'int1':
        t = dict(x=_ints(xs, 901), w=_ints(ws, 902), bias=_ints((cout,), 903), dy=_ints(ys, 904))
        for key in ('x', 'w', 'dy'):
            t[key].reshape(-1)[5] = 4.0
    else:
        t = dict(x=_int2(xs, 911, 1.0), w=_int2(ws, 912, 1.0), bias=4096.0 * _ints((cout,), 913), dy=_int2(ys, 914, 0.3))
    return {k: v.float() for k, v in t.items()}


def _convt(x, w, dy):
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv_transpose3d(xr, wr, None, stride=(1, 2, 2), padding=(0, 1, 1))
    gx, gw = torch.autograd.grad(y, (xr, wr), dy)
    return y.detach(), gx, gw


def convt_reference(t, from_planes):
    """fp64 y, dx, dw, db of the transposed convolution: of the values themselves, or what the split kernels compute from the planes."""
    b = t['bias'].double().reshape(1, -1, 1, 1, 1)
    db = t['dy'].double().sum(dim=(0, 2, 3, 4))
    if not from_planes:
        y, gx, gw = _convt(t['x'].double(), t['w'].double(), t['dy'].double())
        return {'y': y + b, 'dx': gx, 'dw': gw, 'db': db}
    (xh, xl, sx), (wh, wl, sw), (gh, gl, sg) = planes(t['x']), planes(t['w']), planes(t['dy'])
    y = (_convt(xh, wh + wl, gh)[0] + _convt(xl, wh, gh)[0]) / (sx * sw)
    gx = (_convt(xh, wh + wl, gh)[1] + _convt(xh, wh, gl)[1]) / (sg * sw)
    gw = (_convt(xh + xl, wh, gh)[2] + _convt(xh, wh, gl)[2]) / (sg * sx)
    return {'y': y + b, 'dx': gx, 'dw': gw, 'db': db}


def convt_exactness(t, family):
    """max sum |terms| / unit per output kind (see exactness())."""
    (xh, xl, sx), (wh, wl, sw), (gh, gl, sg) = planes(t['x']), planes(t['w']), planes(t['dy'])
    a = torch.abs
    unit, post = (2.0 ** 24, 1.0) if family == 'int1' else (2.0 ** 16, 4096.0)
    y, gx, gw = _convt(a(xh) + a(xl), a(wh) + a(wl), a(gh) + a(gl))
    return {'y': float((y / unit + a(t['bias'].double()).reshape(1, -1, 1, 1, 1) / post).max()), 'dx': float(gx.max() / unit),
            'dw': float(gw.max() / unit), 'db': float(a(t['dy'].double()).sum(dim=(0, 2, 3, 4)).max())}
