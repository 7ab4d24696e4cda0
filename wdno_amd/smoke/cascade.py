"""The conditions of the space super-resolution level on the GPU: what InferencePipeline.run_super_model (smoke/inference_2d.py:176-196) hands
to the super model's sample() as low, init / RESCALER[-2] and control / RESCALER[24:40], written as the sampler's condition source
[B, pad_t, 82, pad_x, pad_x] in network units by two launches: the packed 3-D analysis of the two fine control fields, and
csrc/smoke_cascade.hip (include/wdno_hip.h: wdno_smoke_cascade_conditions), which writes every element of the source.

The reference builds these with tensor_to_coef / coef_to_tensor round trips of the base sample, an expand + reshape up-sampling, a 2-D and a
3-D transform, two paddings per condition, three divisions and, inside sample(), three copies into a zeroed tensor. Here the base sample is
read in place through its strides, the nearest x2, the replicate rim, the zero padding and the divisions happen in the store, and
GaussianDiffusion.sample_with_source(src, ...) takes the tensor as it is.

The fused analysis that stores straight into the state (wdno_dwt_fwd_packed) writes 16-byte aligned rows; the control block of this level
starts at row 1, column 1, which no aligned store reaches, so the analysis goes into its own coefficient tensor [B, 2, 8, t1, h1, w1] (11 MB
at batch 8, full size, against the 101 MB source) and the conditions launch reads it.

super_conditions() -- the launches on torch's current stream; on CPU tensors the same values in plain torch (the route of the CPU tests).
views()            -- (low, init, control) as views of the source, for sample(low=, init=, control=) and sample_with_source.
plan()             -- pure Python: the descriptor's integers, the grid and the LDS bytes; needs neither the library nor a GPU.

Frame order of init. At this level the reference shows sub-band f % 4 in frame f (l.181: unsqueeze(1).expand(B, pad_t / 4, 4, ...)), not
sub-band f // (pad_t / 4) as run_model does at the base level (l.247) and as the training data has it. It is a quirk of the reference that
this drop-in keeps.
"""
import ctypes as C

import torch
import torch.nn.functional as F

from wdno_amd.smoke.guidance import SUPPORTED

CHANNELS = 82
BANDS3 = ('aaa', 'aad', 'ada', 'add', 'daa', 'dad', 'dda', 'ddd')


def views(src):
    """(low [B, pad_t, 40, pad_x, pad_x], init [B, pad_t, pad_x, pad_x], control [B, pad_t, 16, pad_x, pad_x]) of a condition source."""
    return src[:, :, 40:80], src[:, :, -2], src[:, :, 24:40]


def plan(prev_shape, prev_block, fine_hw, shape1, pad_t=24, pad_x=80, wave_type='bior1.3', pad_mode='zero', strides=None, rho_strides=None):
    """Host integers of one wdno_smoke_cascade_conditions call: the base sample of prev_shape = (B, F0, C0, H0, W0) with element `strides`
    (default: contiguous) and coefficient block prev_block = (t0, h0, w0), the fine initial density of fine_hw = (Hf, Wf) cells with
    rho_strides = (sample, row, column), the fine block shape1 = (t1, h1, w1). ValueError for whatever the kernel cannot walk."""
    from wdno_amd.filters import filter_bank
    if (wave_type, pad_mode) not in SUPPORTED:
        raise ValueError(f'smoke cascade conditions: (wave, mode) = ({wave_type!r}, {pad_mode!r}) is not built; supported: {sorted(SUPPORTED)}')
    L = len(filter_bank(wave_type)[0])
    B, F0, C0, H0, W0 = (int(v) for v in prev_shape)
    t0, h0, w0 = (int(v) for v in prev_block)
    t1, h1, w1 = (int(v) for v in shape1)
    Hf, Wf = (int(v) for v in fine_hw)
    pad_t, pad_x = int(pad_t), int(pad_x)
    if pad_t < 4 or pad_t % 4 or pad_x < 4 or pad_x % 4:
        raise ValueError(f'smoke cascade conditions: pad_t = {pad_t} and pad_x = {pad_x} must be multiples of 4 (four sub-bands over the frames; 16-byte rows)')
    if C0 < 40:
        raise ValueError(f'smoke cascade conditions: the base sample has {C0} channels; 40 coefficient channels are needed')
    if not (1 <= t0 <= min(F0, pad_t) and 1 <= h0 <= H0 and 1 <= w0 <= W0):
        raise ValueError(f'smoke cascade conditions: base block {(t0, h0, w0)} does not fit the {(F0, H0, W0)} sample or the {pad_t} frames')
    if 2 * h0 != h1 + 2 or 2 * w0 != w1 + 2:
        raise ValueError(f'smoke cascade conditions: twice the base block {(h0, w0)} is not the fine block {(h1, w1)} plus its rim of one')
    if not (1 <= t1 <= pad_t and h1 >= 1 and w1 >= 1 and h1 + 2 <= pad_x and w1 + 2 <= pad_x):
        raise ValueError(f'smoke cascade conditions: fine block {(t1, h1, w1)} at offset 1 with its rim does not fit ({pad_t}, {pad_x}, {pad_x})')
    if h1 != (Hf + L - 1) // 2 or w1 != (Wf + L - 1) // 2:
        raise ValueError(f'smoke cascade conditions: the analysis of a {(Hf, Wf)} density is not {(h1, w1)} coefficients')
    ss, fs, cs, rs, es = (F0 * C0 * H0 * W0, C0 * H0 * W0, H0 * W0, W0, 1) if strides is None else (int(v) for v in strides)
    rss, rrs, res = (Hf * Wf, Wf, 1) if rho_strides is None else (int(v) for v in rho_strides)
    if es != 1 or rs < W0 or cs < H0 * rs or fs < C0 * cs or ss < F0 * fs or ss >= 2 ** 31:
        raise ValueError(f'smoke cascade conditions: strides {(ss, fs, cs, rs, es)} of a {tuple(prev_shape)} sample: columns must be contiguous, the '
                         'axes nested in the order sample, frame, channel, row, and a sample inside 32 bits')
    if res != 1 or rrs < Wf or rss < Hf * rrs or rss >= 2 ** 31:
        raise ValueError(f'smoke cascade conditions: strides {(rss, rrs, res)} of the {(Hf, Wf)} density are outside what the kernel walks')
    if B < 1 or B > 65535 or B * pad_t >= 2 ** 31 or pad_x >= 4096 or pad_t * CHANNELS * pad_x * pad_x >= 2 ** 31:
        raise ValueError(f'smoke cascade conditions: batch {B} of ({pad_t}, {CHANNELS}, {pad_x}, {pad_x}) is outside the kernel\'s grid / 32-bit strides')
    return dict(prev_sample_stride=ss, rho_sample_stride=rss, prev_frame_stride=fs, prev_chan_stride=cs, prev_row_stride=rs, rho_row_stride=rrs,
                B=B, F0=F0, C0=C0, H0=H0, W0=W0, t0=t0, h0=h0, w0=w0, t1=t1, h1=h1, w1=w1, Hf=Hf, Wf=Wf, pad_t=pad_t, pad_x=pad_x, C=CHANNELS,
                L=L, mode=1, grid=(B * pad_t, CHANNELS), lds_bytes=4 * 2 * L)


# ----------------------------------------------------------------------------------------------------- plain torch (CPU tensors)
def _analysis(x, taps, axis):
    """Zero-mode analysis along `axis`: y[k] = sum_m dec[L - 1 - m] x[2 k + m - p], p = (2 L - 3) // 2, (N + L - 1) // 2 samples."""
    x = x.movedim(axis, -1)
    L, N = len(taps), x.shape[-1]
    p, nk = (2 * L - 3) // 2, (N + L - 1) // 2
    xp = F.pad(x, (p, p + N % 2 + 2))
    y = 0
    for m in range(L):
        y = y + float(taps[L - 1 - m]) * xp[..., m:m + 2 * nk:2]
    return y.movedim(-1, axis)


def _torch_conditions(prev, prev_block, fields, r, shape1, pad_t, pad_x, wave_type):
    from wdno_amd.filters import filter_bank
    dl, dh = filter_bank(wave_type)[:2]
    t0, h0, w0 = prev_block
    t1, h1, w1 = shape1
    B = prev.shape[0]
    low = prev[:, :t0, :40, :h0, :w0].repeat_interleave(2, dim=3).repeat_interleave(2, dim=4)
    low = F.pad(low, (0, pad_x - 2 * w0, 0, pad_x - 2 * h0, 0, 0, 0, pad_t - t0))
    ctrl = fields[:, :, 3:5].permute(0, 2, 1, 3, 4)                                        # [B, 2, T, H, W]
    bands = []
    for key in BANDS3:
        y = ctrl
        for ax, letter in zip((-3, -2, -1), key):
            y = _analysis(y, dl if letter == 'a' else dh, ax)
        bands.append(y)
    coef = torch.stack(bands, dim=2)                                                       # [B, 2, 8, t1, h1, w1]
    assert tuple(coef.shape[-3:]) == (t1, h1, w1), (tuple(coef.shape), shape1)
    control = F.pad(coef.reshape(-1, t1, h1, w1), (1, 1, 1, 1), mode='replicate')
    control = F.pad(control, (0, pad_x - w1 - 2, 0, pad_x - h1 - 2, 0, pad_t - t1)).reshape(B, 16, pad_t, pad_x, pad_x).permute(0, 2, 1, 3, 4)
    rho = fields[:, 0, 0]
    lo_w, hi_w = _analysis(rho, dl, -1), _analysis(rho, dh, -1)
    sub = torch.stack((_analysis(lo_w, dl, -2), _analysis(lo_w, dh, -2), _analysis(hi_w, dl, -2), _analysis(hi_w, dh, -2)), dim=1)
    init = sub.unsqueeze(1).expand(B, pad_t // 4, 4, h1, w1).reshape(B, pad_t, h1, w1)       # frame f shows sub-band f % 4 (l.181)
    init = F.pad(init, (0, pad_x - w1, 0, pad_x - h1))
    src = torch.zeros(B, pad_t, CHANNELS, pad_x, pad_x, dtype=torch.float32)
    src[:, :, 40:80] = low
    src[:, :, 24:40] = control / r[24:40].reshape(1, 1, 16, 1, 1)
    src[:, :, -2] = init / r[-2]
    return src


_filt = {}


def super_conditions(prev_sample, prev_shape, fields_fine, rescaler, shape1, pad_t=24, pad_x=80, wave_type='bior1.3', pad_mode='zero'):
    """The condition source [B, pad_t, 82, pad_x, pad_x] (fp32, network units) of the super level. prev_sample [B, F0, C0 >= 40, H0, W0]: the base
    level's sample (network units; a view whose columns are contiguous is read in place), prev_shape its coefficient block (t0, h0, w0);
    fields_fine [B, T, >= 5, H, W]: the state at the fine grid, not rescaled (field 0 at frame 0 is the initial density, fields 3 and 4 the
    controls); rescaler: the 82 values in any shape; shape1 = (t1, h1, w1): the fine coefficient block. See views()."""
    from wdno_amd import _lib
    from wdno_amd.filters import filter_bank
    B, T, _, Hf, Wf = (int(v) for v in fields_fine.shape)
    r = torch.as_tensor(rescaler, dtype=torch.float32).reshape(-1)
    if r.numel() != CHANNELS:
        raise ValueError(f'smoke cascade conditions: RESCALER has {r.numel()} entries, the super model {CHANNELS} channels')
    if prev_sample.dim() != 5 or prev_sample.shape[0] != B or prev_sample.dtype != torch.float32 or fields_fine.dtype != torch.float32:
        raise ValueError(f'smoke cascade conditions: base sample {tuple(prev_sample.shape)} {prev_sample.dtype} against fine state '
                         f'{tuple(fields_fine.shape)} {fields_fine.dtype}: float32 tensors of one batch are needed')
    prev_shape, shape1 = tuple(int(v) for v in prev_shape), tuple(int(v) for v in shape1)
    prev = prev_sample.detach()
    st = list(prev.stride())
    if B == 1:
        st[0] = prev.shape[1] * st[1]            # the stride of a one-sample axis is never walked
    rho = fields_fine[:, 0, 0]
    if rho.stride(-1) != 1:
        rho = rho.contiguous()
    rst = [Hf * rho.stride(1) if B == 1 else rho.stride(0), rho.stride(1), 1]
    try:
        pl = plan(tuple(prev.shape), prev_shape, (Hf, Wf), shape1, pad_t, pad_x, wave_type, pad_mode, strides=st, rho_strides=rst)
    except ValueError:
        if prev.is_contiguous() and rho.is_contiguous():
            raise
        prev, rho = prev.contiguous(), rho.contiguous()       # views the kernel cannot walk: one copy each
        pl = plan(tuple(prev.shape), prev_shape, (Hf, Wf), shape1, pad_t, pad_x, wave_type, pad_mode)
    if not prev.is_cuda:
        return _torch_conditions(prev, prev_shape, fields_fine.detach(), r, shape1, pad_t, pad_x, wave_type)
    from wdno_amd import wavelets as Wv
    from wdno_amd.ops import _p, _stream
    if fields_fine.device != prev.device:
        raise ValueError(f'smoke cascade conditions: base sample on {prev.device}, fine state on {fields_fine.device}')
    pl.pop('grid'), pl.pop('lds_bytes')
    filt = _filt.get(wave_type)
    if filt is None:
        vals = [float(v) for bank in filter_bank(wave_type) for v in bank]
        filt = _filt[wave_type] = (C.c_float * len(vals))(*vals)
    with torch.cuda.device(prev.device):
        ctrl = fields_fine.detach()[:, :, 3:5].permute(0, 2, 1, 3, 4).reshape(B * 2, T, Hf, Wf).contiguous()
        coef = Wv.dwt_packed(ctrl, wave_type, pad_mode, 3)                                  # [B 2, 8, t1, h1, w1]
        if tuple(coef.shape[-3:]) != shape1:
            raise ValueError(f'smoke cascade conditions: the analysis of {(T, Hf, Wf)} fields is {tuple(coef.shape[-3:])}, the fine block {shape1}')
        r = r.to(prev.device).contiguous()
        src = torch.empty((B, pad_t, CHANNELS, pad_x, pad_x), dtype=torch.float32, device=prev.device)
        desc = _lib.SmokeCascadeDesc(**pl)
        _lib.check(_lib.load().wdno_smoke_cascade_conditions(_p(prev), _p(coef), _p(rho), _p(r), _p(src), C.byref(desc), filt, _stream()),
                   'wdno_smoke_cascade_conditions')
    return src
