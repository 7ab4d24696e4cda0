"""Autograd-aware wrappers around the C ABI (include/wdno_hip.h).

PyTorch is used for device memory, streams and the autograd tape only; every forward / backward body below is one
or more launches of libwdno_hip.so. Activations are channels-last ("CL"): [N, (D,) H, W, C] with C padded to a
multiple of 4. There is no CPU path: non-CUDA tensors raise.
"""
import contextlib
import ctypes as C
import math
import os

import torch

from . import _lib
from ._lib import AttnDesc, CondDesc, ConvGeom, DwtDesc

WEIGHT_EPOCH = 0          # bumped by wdno_amd.trainer after every in-place optimiser step (invalidates packed weights)
_pack_cache = {}


PROFILE = None            # bench.py sets this to a dict: kernel symbol -> list of (start_event, end_event, flops)


class _timed:
    """Brackets one launch with HIP events on the current stream when bench.py has switched profiling on."""

    def __init__(self, key, flops):
        self.key, self.flops = key, flops

    def __enter__(self):
        if PROFILE is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *a):
        if PROFILE is not None:
            self.e1.record()
            PROFILE.setdefault(self.key, []).append((self.e0, self.e1, self.flops))
        return False


PARAM_EPOCH = 0           # bumped only when parameter VALUES may have changed behind autograd's version counters (not by cache evictions)


def bump_weight_epoch(params=True):
    """params=False: only the operand caches were dropped / marked stale (the parameters themselves hold the same values)."""
    global WEIGHT_EPOCH, PARAM_EPOCH
    WEIGHT_EPOCH += 1
    if params:
        PARAM_EPOCH += 1


def _param_epoch(p):
    """What a backward that re-reads tables derived from parameter p compares: the global value epoch (checkpoint loads, EMA copies) and
    the epoch of the flat buffer that owns p (trainer.FlatBuffers.params_changed) -- another model's optimiser step does not count."""
    cell = getattr(p, '_wdno_epoch_cell', None)
    return (PARAM_EPOCH, -1 if cell is None else cell[0])


def drop_weight_caches():
    """Forget every packed / split weight operand (they hold references to the parameter storages they were built from)."""
    _pack_cache.clear()
    _wplans.clear()
    _wtables.clear()
    bump_weight_epoch(params=False)


def _lib_():
    return _lib.load()


def _p(t):
    return None if t is None else t.data_ptr()      # ctypes takes a plain int for a c_void_p argument


_raw_stream = torch._C._cuda_getCurrentRawStream     # torch.cuda.current_stream() costs ~3 us of host time per launch
_cur_device = torch._C._cuda_getDevice


def _stream():
    return _raw_stream(_cur_device())


def _chk(t, name='tensor'):
    if not t.is_cuda:
        raise RuntimeError(f'wdno_amd: {name} must live on the GPU (no CPU fallback on the hot path)')
    if t.dtype != torch.float32:
        raise RuntimeError(f'wdno_amd: {name} must be float32, got {t.dtype}')
    return t if t.is_contiguous() else t.contiguous()


def _chk_act(t, name='tensor'):
    """An activation that may be bf16 storage (single-product mode: the output of a convolution in front of a GroupNorm, ops.ACT16)."""
    if t.dtype != torch.bfloat16:
        return _chk(t, name)
    if not t.is_cuda:
        raise RuntimeError(f'wdno_amd: {name} must live on the GPU (no CPU fallback on the hot path)')
    return t if t.is_contiguous() else t.contiguous()


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def pad4(c):
    return (c + 3) // 4 * 4


# ----------------------------------------------------------------------------------------------------- layout
class _NcToCl(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cp):
        x = _chk(x, 'x')
        n, c = x.shape[0], x.shape[1]
        sp = tuple(x.shape[2:])
        s = int(math.prod(sp))
        out = torch.empty((n, *sp, cp), device=x.device, dtype=torch.float32)
        _lib.check(_lib_().wdno_nc_to_cl(_p(x), _p(out), n, c, s, cp, _stream()), 'nc_to_cl')
        ctx.c = c
        return out

    @staticmethod
    def backward(ctx, g):
        return cl_to_nc_raw(_chk(g, 'grad'), ctx.c), None


def cl_to_nc_raw(x, c):
    n, cp = x.shape[0], x.shape[-1]
    sp = tuple(x.shape[1:-1])
    s = int(math.prod(sp))
    out = torch.empty((n, c, *sp), device=x.device, dtype=torch.float32)
    _lib.check(_lib_().wdno_cl_to_nc(_p(x), _p(out), n, c, s, cp, _stream()), 'cl_to_nc')
    return out


class _ClToNc(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, c):
        x = _chk(x, 'x')
        ctx.cp = x.shape[-1]
        return cl_to_nc_raw(x, c)

    @staticmethod
    def backward(ctx, g):
        g = _chk(g, 'grad')
        n, c = g.shape[0], g.shape[1]
        sp = tuple(g.shape[2:])
        out = torch.empty((n, *sp, ctx.cp), device=g.device, dtype=torch.float32)
        _lib.check(_lib_().wdno_nc_to_cl(_p(g), _p(out), n, c, int(math.prod(sp)), ctx.cp, _stream()), 'nc_to_cl')
        return out, None


def nc_to_cl(x, cp=None):
    """[N, C, *spatial] -> [N, *spatial, Cp] (zero-padded channels)."""
    return _NcToCl.apply(x, pad4(x.shape[1]) if cp is None else cp)


def cl_to_nc(x, c):
    """[N, *spatial, Cp] -> [N, C, *spatial]."""
    return _ClToNc.apply(x, c)


class _Concat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, planes_only=False):
        ra, rb = _known_amax(a), _known_amax(b)
        a, b = _chk(a, 'a'), _chk(b, 'b')
        ca, cb = a.shape[-1], b.shape[-1]
        p = a.numel() // ca
        out = torch.empty((*a.shape[:-1], ca + cb), device=a.device, dtype=torch.float32)
        ctx.ca, ctx.cb = ca, cb
        if (planes_only and PLANES_FWD and CONV_MATH in ('f16x3', 'bf16') and ca % 8 == 0 and cb % 8 == 0
                and (_lp() or (ra is not None and rb is not None))):
            # the caller states that only convolutions reading planes use the result: `out` stays unwritten
            hi = torch.empty((p, ca + cb), device=a.device, dtype=torch.float16)
            lo = sc = None
            if not _lp():
                lo = torch.empty((p, ca + cb), device=a.device, dtype=torch.float16)
                sc = torch.empty((1,), device=a.device, dtype=torch.float32)
            _lib.check(_lib_().wdno_concat2_cl_planes(_p(a), ca, _p(b), cb, _p(ra), _p(rb), _p(hi), _p(lo), _p(sc), p, _stream()), 'concat2_planes')
            return _planes_only(out, (hi, lo, sc))
        rec = _new_amax_record(a.device)
        _lib.check(_lib_().wdno_concat2_cl_amax(_p(a), ca, _p(b), cb, _p(out), _p(rec), p, _stream()), 'concat2_cl')
        return _leave_amax(out, rec)

    @staticmethod
    def backward(ctx, g):
        g = _chk(g, 'grad')
        ca, cb = ctx.ca, ctx.cb
        p = g.numel() // (ca + cb)
        ga = torch.empty((*g.shape[:-1], ca), device=g.device, dtype=torch.float32)
        gb = torch.empty((*g.shape[:-1], cb), device=g.device, dtype=torch.float32)
        _lib.check(_lib_().wdno_split2_cl(_p(g), _p(ga), ca, _p(gb), cb, p, _stream()), 'split2_cl')
        return ga, gb, None


def concat_cl(a, b, planes_only=False):
    """(a | b) along the channel axis. planes_only: the caller states that the result is read only by convolutions that take fp16 planes
    (conv_reads_planes for every reader); where the amax records of a and b are known it then exists only as those planes."""
    return _Concat.apply(a, b, planes_only)


def resnet_reads_planes(x_pixels, block):
    """Do both readers of a ResnetBlock's input -- block1's convolution and the 1 x 1 skip projection -- take fp16 planes?"""
    rc = getattr(block, 'res_conv', None)
    return (rc is not None and hasattr(rc, 'weight') and conv_reads_planes(x_pixels, block.block1.proj.weight)
            and conv_reads_planes(x_pixels, rc.weight))


class _Up2x(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _chk(x, 'x')
        n, h, w, c = x.shape
        out = torch.empty((n, 2 * h, 2 * w, c), device=x.device, dtype=torch.float32)
        _lib.check(_lib_().wdno_upsample2x_cl_fwd(_p(x), _p(out), n, h, w, c, _stream()), 'upsample2x_fwd')
        return out

    @staticmethod
    def backward(ctx, g):
        g = _chk(g, 'grad')
        n, h2, w2, c = g.shape
        out = torch.empty((n, h2 // 2, w2 // 2, c), device=g.device, dtype=torch.float32)
        _lib.check(_lib_().wdno_upsample2x_cl_bwd(_p(g), _p(out), n, h2 // 2, w2 // 2, c, _stream()), 'upsample2x_bwd')
        return out


def upsample2x_cl(x):
    return _Up2x.apply(x)


# ----------------------------------------------------------------------------------------------------- pointwise
class _Act(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kind):
        x = _chk(x, 'x')
        y = torch.empty_like(x)
        _lib.check(_lib_().wdno_act_fwd(_p(x), _p(y), x.numel(), kind, _stream()), 'act_fwd')
        ctx.save_for_backward(x)
        ctx.kind = kind
        return y

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        g = _chk(g, 'grad')
        dx = torch.empty_like(x)
        _lib.check(_lib_().wdno_act_bwd(_p(x), _p(g), _p(dx), x.numel(), ctx.kind, _stream()), 'act_bwd')
        return dx, None


def silu(x):
    return _Act.apply(x, 0)


def gelu(x):
    return _Act.apply(x, 1)


class _Add(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = _chk(a, 'a'), _chk(b, 'b')
        assert a.shape == b.shape
        out = torch.empty_like(a)
        rec = _new_amax_record(a.device)
        _lib.check(_lib_().wdno_add_amax(_p(a), _p(b), _p(out), _p(rec), a.numel(), _stream()), 'add')
        return _leave_amax(out, rec)

    @staticmethod
    def backward(ctx, g):
        return g, g


def add(a, b):
    return _Add.apply(a, b)


def silu_shared(t):
    """silu(t), computed once per tensor (and version): every ResnetBlock applies the same SiLU to the same time embedding in front of its
    own projection (conv3d.py:118-133, unet.py:151-165) -- one activation forward and backward per step instead of one per block."""
    h = getattr(t, '_wdno_silu', None)
    if h is not None and h[1] == t._version and h[2] == torch.is_grad_enabled():
        return h[0]
    a = silu(t)
    try:
        t._wdno_silu = (a, t._version, torch.is_grad_enabled())
    except Exception:
        pass
    return a


_freq_cache = {}


def sinusoidal_embedding(t, dim, theta=10000.0):
    """[B] int64 -> [B, dim] (no gradient: timesteps are integers). The frequency table is built once on the host
    with the same torch CPU arithmetic the reference uses, so the fp32 arguments t*f are bit-identical to it."""
    t = t.to(torch.int64).contiguous()
    if not t.is_cuda:
        raise RuntimeError('wdno_amd: timesteps must live on the GPU')
    key = (dim, float(theta), str(t.device))
    if key not in _freq_cache:
        half = dim // 2
        _freq_cache[key] = torch.exp(torch.arange(half) * -(math.log(theta) / (half - 1))).to(torch.float32).to(t.device)
    out = torch.empty((t.shape[0], dim), device=t.device, dtype=torch.float32)
    _lib.check(_lib_().wdno_sinusoidal_emb(_p(t), _p(_freq_cache[key]), _p(out), t.shape[0], dim, _stream()), 'sinusoidal_emb')
    return out


# ----------------------------------------------------------------------------------------------------- convolution
def _geom(x_shape, c, k, ks, st, pd, out_sp, y_sp=None, ostride=(1, 1, 1), ooff=(0, 0, 0)):
    n, d, h, w = x_shape
    y_sp = out_sp if y_sp is None else y_sp
    return ConvGeom(n, d, h, w, c, out_sp[0], out_sp[1], out_sp[2], k, ks[0], ks[1], ks[2], st[0], st[1], st[2],
                    pd[0], pd[1], pd[2], y_sp[0], y_sp[1], y_sp[2], ostride[0], ostride[1], ostride[2],
                    ooff[0], ooff[1], ooff[2])


def _as5(w):
    """Reference weight layouts -> [K, C, kd, kh, kw]."""
    if w.dim() == 2:
        return w[:, :, None, None, None]
    if w.dim() == 4:
        return w[:, :, None]
    return w


def _cached(w, kind, cp, kp, build):
    """Packed-weight cache. The entry keeps a reference to the weight's storage, so its address cannot be recycled by
    another tensor while the entry is alive (a recycled address with equal shape/version would be a stale hit)."""
    key = (w.data_ptr(), kind, cp, kp, tuple(w.shape), tuple(w.stride()))
    ver = (w._version, WEIGHT_EPOCH)
    hit = _pack_cache.get(key)
    if hit is not None and hit[0] == ver:
        return hit[1]
    with torch.no_grad():
        packed = build().contiguous()
    if len(_pack_cache) > 4096:
        _pack_cache.clear()
        bump_weight_epoch(params=False)          # captured graphs replay pointers into the dropped operands: the epoch is part of their cache key
    _pack_cache[key] = (ver, packed, w.detach())
    return packed


def _padded(w5, kp, cp):
    k, c = w5.shape[0], w5.shape[1]
    if k == kp and c == cp:
        return w5
    out = w5.new_zeros((kp, cp, *w5.shape[2:]))
    out[:k, :c] = w5
    return out


def pack_fwd(w, cp, kp):
    """[K, C, kd, kh, kw] -> [kd, kh, Kp, kw, Cp]"""
    return _cached(w, 'f', cp, kp, lambda: _padded(_as5(w.detach()), kp, cp).permute(2, 3, 0, 4, 1))


def pack_dgrad(w, cp, kp):
    """stride-1 data gradient: dx = conv(dy, flipped/transposed w): [kd, kh, Cp, kw, Kp]"""
    return _cached(w, 'd', cp, kp, lambda: _padded(_as5(w.detach()), kp, cp).flip(2, 3, 4).permute(2, 3, 1, 4, 0))


def pack_transposed(w_io, cin_p, cout_p):
    """k=(1,4,4), s=(1,2,2), p=(0,1,1) transposed convolution, weight [in, out, 1, 4, 4]:
    four parity classes (py, px), each a (1,2,2) stride-1 convolution: -> [2, 2][1, 2, Cout_p, 2, Cin_p]
    with wt[py][px][0][dy][o][dx][i] = w[i][o][0][3 - py - 2 dy][3 - px - 2 dx]."""
    def build():
        w = w_io.detach()
        cin, cout = w.shape[0], w.shape[1]
        out = w.new_zeros((2, 2, 1, 2, cout_p, 2, cin_p))
        for py in range(2):
            for px in range(2):
                for dy in range(2):
                    for dx in range(2):
                        out[py, px, 0, dy, :cout, dx, :cin] = w[:, :, 0, 3 - py - 2 * dy, 3 - px - 2 * dx].t()
        return out
    return _cached(w_io, 't', cin_p, cout_p, build)


# 'f16x3' = fp32-equivalent 3 x fp16-split MFMA for the large convolutions (forward and data gradient); 'f32' = exact-fp32
# MFMA everywhere. Small problems always take the exact kernel.
# 'bf16' = BASELINE.json configs[1]: one bf16 plane per operand and ONE product on v_mfma_f32_32x32x16_bf16, fp32 master weights and
# accumulators (the reference's knob: Trainer(amp=True), train_diffusion.py:62,71-74). bf16-class accuracy, see tests/test_gpu_bf16.py.
CONV_MATH = os.environ.get('WDNO_CONV_MATH', 'f16x3')
LOWP_AVAILABLE = True


def _lp():
    return CONV_MATH == 'bf16'


@contextlib.contextmanager
def _math(mode):
    """Run a block of launches under another convolution arithmetic (the fused attention blocks keep their split-fp16 projections when
    the convolutions around them run on single bf16 planes)."""
    global CONV_MATH
    prev, CONV_MATH = CONV_MATH, mode
    try:
        yield
    finally:
        CONV_MATH = prev
H3_MIN_PIXELS = 1024
PATCH_DGRAD_H3 = True     # data gradient of the folded (1,2,2)/s2 Downsample on the split-fp16 kernels (test knob; False = four exact-fp32 launches)
H3_MIN_REDUCTION = 64


def pad8(c):
    return (c + 7) // 8 * 8


_amax_pool = {}
AMAX_FLOATS = 64 * 16    # WDNO_AMAX_FLOATS
AMAX_HINTS = True         # producers leave amax records on the tensors they write (test knob: results are bit-identical without)


# Hand-over forms between layers. These were environment A/B switches while each form was being measured (every one
# won its same-box A/B); the environment variables are gone -- the product has ONE path -- and two module attributes remain as TEST knobs:
# the planes-vs-fp32 equivalence tests (tests/test_gpu_ops.py::test_*_planes*) evaluate a layer both ways and compare.
PLANES_FWD = True         # norm / attention layers in front of a convolution write its fp16 planes (test knob)
GRAD_PLANES = True        # GroupNorm / attention backward write the fp16 planes of the gradient the convolution in front reads (test knob)
_CAPTURE = None          # [pool, next index] while a HIP graph is being captured through graph_capture()


@contextlib.contextmanager
def graph_capture(graph, stream=None):
    """`torch.cuda.graph(graph)` for launches of this library. Everything the library needs per launch is either a kernel
    argument or device memory, so a captured step replays unchanged; the one piece of state that eager execution renews per
    launch -- the zeroed amax records -- comes, during a capture, from a pool that is allocated AND zero-filled inside the
    graph: every replay starts from zeroed records exactly like an eager step, and replays are bit-identical to eager runs.
    Run the step once eagerly first (packed / split weight operands and pixel tables are built on first use)."""
    global _CAPTURE
    assert _CAPTURE is None, 'nested graph captures are not supported'
    # capture_error_mode 'thread_local': only THIS thread is held to the capture rules. Under the default ('global') any thread that touches the
    # HIP API in a capture-unsafe way fails -- and a process group's watchdog thread polls the events of earlier collectives (hipEventQuery) whenever
    # it wakes up: a capture that follows eager data-parallel steps then dies with "operation not permitted when stream is capturing" a few times in
    # a hundred (tests/test_gpu_distributed.py caught it on a one-rank RCCL group). Launches of other threads INTO the capturing stream -- autograd's
    # worker thread running the backward -- are recorded in every mode.
    with torch.cuda.graph(graph, stream=stream, capture_error_mode='thread_local'):
        _CAPTURE = [None, 0]
        try:
            yield graph
        finally:
            _CAPTURE = None


def _amax_slot(device):
    """A zeroed amax record (AMAX_FLOATS floats whose maximum will be max|x|, include/wdno_hip.h) from a pool. An exhausted
    pool is replaced, never re-zeroed: records left on tensors by their producers (_leave_amax) may still be read."""
    if _CAPTURE is not None:
        st = _CAPTURE
        if st[0] is None or st[1] >= st[0].shape[0]:
            st[0], st[1] = torch.zeros((1024, AMAX_FLOATS), device=device, dtype=torch.float32), 0      # a captured fill: redone by every replay
        rec = st[0][st[1]]
        st[1] += 1
        return rec
    key = str(device)
    st = _amax_pool.get(key)
    if st is None or st[1] >= st[0].shape[0]:
        st = [torch.zeros((1024, AMAX_FLOATS), device=device, dtype=torch.float32), 0]
        _amax_pool[key] = st
    rec = st[0][st[1]]
    st[1] += 1
    return rec


def _new_amax_record(device):
    return _amax_slot(device) if AMAX_HINTS and not _lp() else None          # bf16 planes carry no scale


def _leave_amax(t, rec):
    """The kernel that wrote t also filled `rec` with its amax: remember it on the tensor object together with the tensor's
    version, so that a later in-place change (autograd accumulating another gradient into it) voids the record."""
    if rec is not None:
        t._wdno_amax = (rec, t._version)
    return t


def _known_amax(t):
    h = getattr(t, '_wdno_amax', None)
    return h[0] if h is not None and h[1] == t._version and AMAX_HINTS else None


def tensor_amax(x):
    amax = _amax_slot(x.device)
    _lib.check(_lib_().wdno_amax_record(_p(x), x.numel(), _p(amax), _stream()), 'amax')
    return amax


def split_f16_of(t, x2d, amax=None, c8=None):
    """split_f16(x2d) for the rows of tensor t, remembered on t (with its version): a tensor that feeds two convolutions -- the
    input of a ResnetBlock with a projection skip -- is split once, and both keep the same planes for their backward."""
    h = getattr(t, '_wdno_planes', None)
    if (h is not None and h[1] == t._version and h[0][0].shape[0] == x2d.shape[0] and h[2] == CONV_MATH
            and (c8 is None or h[0][0].shape[1] == c8)):
        return h[0]
    planes = split_f16(x2d, amax, c8)
    try:
        t._wdno_planes = (planes, t._version, CONV_MATH)
    except Exception:
        pass
    return planes


def split_f16(x2d, amax=None, c8=None):
    """[rows, C] fp32 -> (hi, lo) fp16 [rows, C8] and the device scalar scale: one amax sweep (unless the producer of the
    tensor left its amax record, `amax`) + one split pass. c8: plane width if not pad8(C) (a 7-wide stem pads to whole 16-channel blocks)."""
    rows, c = x2d.shape
    if c8 is None or _lp():
        c8 = pad8(c)
    lib = _lib_()
    if _lp():                    # one bf16 plane (carried in a float16-typed tensor: 16-bit storage, the kernels reinterpret it)
        hi = torch.empty((rows, c8), device=x2d.device, dtype=torch.float16)
        _lib.check(lib.wdno_cast_bf16(_p(x2d), _p(hi), rows, c, c8, _stream()), 'cast_bf16')
        return hi, None, None
    if amax is None:
        amax = tensor_amax(x2d)
    hi = torch.empty((rows, c8), device=x2d.device, dtype=torch.float16)
    lo = torch.empty((rows, c8), device=x2d.device, dtype=torch.float16)
    scale = amax[1:2]            # a float of the record's first line that no slot uses: saves an allocation per split
    _lib.check(lib.wdno_split_f16(_p(x2d), _p(amax), _p(hi), _p(lo), _p(scale), rows, c, c8, _stream()), 'split_f16')
    return hi, lo, scale


def split_f16_colsum(x2d, amax=None, bias=None, k=None):
    """split_f16 that also returns the column sums [C] of x2d from the same pass (bias gradient of a convolution whose dy
    is being split anyway); falls back to split_f16 + colsum for channel counts the fused kernel does not take. bias (the nn.Parameter the
    first k sums are the gradient of): inside a trainer's backward the final sum over the sweep's partial rows is queued for the launch that
    ends the backward (rows_sum_for_param) and the returned sums are the parameter's span of the flat gradient buffer, [k]."""
    rows, c = x2d.shape
    c8 = pad8(c)
    g8 = c8 // 8
    if g8 > 256 or (g8 & (g8 - 1)):
        return split_f16(x2d, amax), colsum(x2d)
    lib = _lib_()
    nb = lib.wdno_split_colsum_ws_bytes(rows, c8)
    ws = _ws(nb, x2d.device)
    flat = None
    if bias is not None and DEFER_ROW_SUMS and _WGRAD_PENDING is not None:
        flat = _flat_grad_out(bias, (k,))
    cs = None if flat is not None else torch.empty(c8, device=x2d.device, dtype=torch.float32)
    if _lp():
        hi = torch.empty((rows, c8), device=x2d.device, dtype=torch.float16)
        _lib.check(lib.wdno_cast_bf16_colsum(_p(x2d), _p(hi), _p(cs), _p(ws), nb, rows, c, c8, _stream()), 'cast_bf16_colsum')
        planes = (hi, None, None)
    else:
        if amax is None:
            amax = tensor_amax(x2d)
        hi = torch.empty((rows, c8), device=x2d.device, dtype=torch.float16)
        lo = torch.empty((rows, c8), device=x2d.device, dtype=torch.float16)
        scale = amax[1:2]
        _lib.check(lib.wdno_split_f16_colsum(_p(x2d), _p(amax), _p(hi), _p(lo), _p(scale), _p(cs), _p(ws), nb, rows, c, c8, _stream()), 'split_f16_colsum')
        planes = (hi, lo, scale)
    if flat is not None:
        return planes, rows_sum_for_param(_RowsJob(ws, ws.data_ptr(), nb // (8 * c8), c8, 0, k, 1), bias, out=flat)
    return planes, cs[:c]


class _WPlan:
    """One packed split-fp16 weight operand that is refreshed every optimiser step: persistent output planes, so the refresh of
    all of them is two multi-tensor launches (wdno_amax_multi, wdno_pack_split_weight_multi) instead of two launches each."""
    __slots__ = ('w', 'wd', 'kind', 'cp8', 'kp', 'hi', 'lo', 'sc', 'ver', 'used', 'lp')


def _wmode(kind):
    """pack mode of csrc/conv_prep.hip: 'f' forward operand, 'd' data-gradient operand, 'p{py}{px}' parity class of a transposed convolution."""
    if kind[0] == 'q':              # tap (py, px) of a (1,2,2) / stride-2 convolution as the data-gradient operand of a 1x1 convolution
        return 6 + 2 * int(kind[1]) + int(kind[2])
    if kind[0] == 'a':              # 'aq' / 'ao': to_qkv / to_out of a temporal attention block in the fragment order of csrc/attn_fused_wide.hip
        return 10 if kind == 'aq' else 11
    return 0 if kind == 'f' else 1 if kind == 'd' else 2 + 2 * int(kind[1]) + int(kind[2])


def _wdims(kind, w5):
    """(K, C, kd, kh, kw) the pack kernel is told for weight w5 (5-D) and operand kind."""
    if kind[0] == 'p':              # ConvTranspose weight [in, out, 1, 4, 4] read as the [out, in, 1, 2, 2] weight of one parity class
        assert tuple(w5.shape[2:]) == (1, 4, 4)
        return w5.shape[1], w5.shape[0], 1, 2, 2
    if kind[0] == 'q':              # [K, C, 1, 2, 2]: one tap of it
        assert tuple(w5.shape[2:]) == (1, 2, 2)
        return w5.shape[0], w5.shape[1], 1, 1, 1
    return tuple(w5.shape)


_wplans = {}            # key -> _WPlan
_wtables = {}           # tuple of plan keys -> (amax buffer, amax table, split table, keep-alive list)


class _AmaxItem(C.Structure):
    _fields_ = [('x', C.c_void_p), ('n', C.c_int64), ('out', C.c_void_p)]


class _WsplitItem(C.Structure):
    _fields_ = [('w', C.c_void_p), ('amax', C.c_void_p), ('hi', C.c_void_p), ('lo', C.c_void_p), ('scale_out', C.c_void_p),
                ('K', C.c_int), ('C', C.c_int), ('kd', C.c_int), ('kh', C.c_int), ('kw', C.c_int), ('A', C.c_int), ('B', C.c_int), ('mode', C.c_int)]


def _refresh_weight_plans(epoch_used, lp=None):
    """Refresh every registered plan that was used in one of the last few weight epochs (they will all be needed again; an
    EMA update also counts as an epoch). lp: which family of operands (single bf16 plane / split fp16 planes); default = the current
    arithmetic. Both exist side by side in the bf16 mode, whose fused attention blocks keep their split-fp16 projections."""
    if lp is None:
        lp = _lp()
    keys = tuple(k for k, pl in _wplans.items() if pl.used >= epoch_used - 3 and pl.wd.is_contiguous() and pl.lp == lp)
    if len(keys) < 2:
        return
    dev = _wplans[keys[0]].wd.device
    tabs = _wtables.get(keys)
    if tabs is None:
        while len(_wtables) >= 8:          # bounded, oldest first; a captured graph that replays an evicted entry holds its own reference (cache_snapshot)
            _wtables.pop(next(iter(_wtables)))
        wptrs = []
        for k in keys:
            pl = _wplans[k]
            if pl.wd.data_ptr() not in wptrs:
                wptrs.append(pl.wd.data_ptr())
        amax = torch.zeros(len(wptrs), device=dev, dtype=torch.float32)
        seen = {}
        aitems = (_AmaxItem * len(wptrs))()
        for k in keys:
            pl = _wplans[k]
            i = wptrs.index(pl.wd.data_ptr())
            if i not in seen:
                seen[i] = True
                aitems[i] = _AmaxItem(pl.wd.data_ptr(), pl.wd.numel(), amax.data_ptr() + 4 * i)
        sitems = (_WsplitItem * len(keys))()
        for j, k in enumerate(keys):
            pl = _wplans[k]
            kk, cc, kd, kh, kw = _wdims(pl.kind, _as5(pl.wd))
            i = wptrs.index(pl.wd.data_ptr())
            if lp:      # one bf16 plane: no amax, no lo plane, no scale
                sitems[j] = _WsplitItem(pl.wd.data_ptr(), None, pl.hi.data_ptr(), None, None, kk, cc, kd, kh, kw, pl.kp, pl.cp8, _wmode(pl.kind))
                continue
            sitems[j] = _WsplitItem(pl.wd.data_ptr(), amax.data_ptr() + 4 * i, pl.hi.data_ptr(), pl.lo.data_ptr(), pl.sc.data_ptr(),
                                    kk, cc, kd, kh, kw, pl.kp, pl.cp8, _wmode(pl.kind))
        at = torch.frombuffer(bytearray(bytes(aitems)), dtype=torch.uint8).to(dev)
        stt = torch.frombuffer(bytearray(bytes(sitems)), dtype=torch.uint8).to(dev)
        tabs = (amax, at, stt, len(wptrs))
        _wtables[keys] = tabs
    amax, at, stt, nw = tabs
    lib = _lib_()
    with torch.no_grad():
        if not lp:
            amax.zero_()
            _lib.check(lib.wdno_amax_multi(_p(at), nw, 64, _stream()), 'amax_multi')      # 64 blocks per weight: 16-byte loads, four in flight per thread
        _lib.check(lib.wdno_pack_split_weight_multi(_p(stt), len(keys), 256, _stream()), 'pack_split_weight_multi')
    for k in keys:
        pl = _wplans[k]
        pl.ver = (pl.w._version, WEIGHT_EPOCH)


def cache_snapshot():
    """Strong references to everything the operand caches hold right now -- packed / split weight planes, the device tables of the
    multi-tensor refresh and of the grouped linear layers, rotary / frequency / pixel tables. A captured HIP graph replays raw device
    pointers into these tensors; the caches themselves evict (size bounds, a changed key set, drop_weight_caches), so whoever owns a
    graph keeps the snapshot for as long as the graph may be replayed (trainer.CapturedStep, diffusion_core._StepGraph)."""
    return [dict(_pack_cache), dict(_wplans), dict(_wtables), dict(_lin_tables), dict(_rot_cache), dict(_pixel_tables), dict(_freq_cache),
            {k: v[0] for k, v in _amax_pool.items()}]


def captured_plans(since=None):
    """The split weight operands a capture used (a graph owner passes them to touch_plans after every replay): those whose `used` epoch
    is at least `since` (the weight epoch the capture started in); without `since`, every operand alive. Operands of other models (the EMA
    copy, a super-resolution model sampled between steps) are not the captured step's and are not re-packed on its account."""
    return [pl for pl in _wplans.values() if since is None or pl.used >= since]


def touch_plans(plans):
    """Replays do not run Python: mark the operands a replayed step used as used in the current weight epoch, so that an eager step that
    follows (a batch of another shape, sampling between steps) refreshes all of them in the usual two launches instead of one by one."""
    e = WEIGHT_EPOCH
    for pl in plans:
        pl.used = e


def prepare_graph_refresh():
    """Before a step is captured in a HIP graph: build the device tables of the two-launch weight refresh NOW (they are uploaded from
    host memory, which a capturing stream does not permit), then mark every operand stale so that the first convolution of the
    captured step records the two refresh launches -- every replay then re-splits all weights before it uses them."""
    epoch = WEIGHT_EPOCH
    for pl in _wplans.values():
        if pl.used >= epoch - 3:              # the operands of the step that has just run eagerly (its optimiser step and an EMA update lie in between)
            pl.used = epoch                   # belong to the step that is about to be captured; another model's (EMA copy, SR model) do not
    bump_weight_epoch(params=False)
    if _wplans:
        for lp in {pl.lp for pl in _wplans.values()}:
            _refresh_weight_plans(WEIGHT_EPOCH, lp)   # eager: tables built (and operands refreshed) outside the capture
    bump_weight_epoch(params=False)


def split_weight(w, kind, cp8, kp, pack=None):
    """Split planes of the packed weight operand (cached per weight version). kind 'f': forward operand
    [kd,kh,kp,kw,cp8]; kind 'd': data-gradient operand [kd,kh,kp(=Cp of x),kw,cp8(=K8 of dy)] with flipped taps.
    The first stale operand met after an optimiser step refreshes ALL operands of the previous step in two launches."""
    lp = _lp()
    key = (w.data_ptr(), kind, cp8, kp, tuple(w.shape), tuple(w.stride()), lp)
    ver = (w._version, WEIGHT_EPOCH)
    pl = _wplans.get(key)
    if pl is not None:
        if pl.ver != ver:
            _refresh_weight_plans(WEIGHT_EPOCH)
        if pl.ver == ver:
            pl.used = WEIGHT_EPOCH
            return pl.hi, pl.lo, pl.sc
    with torch.no_grad():
        wd = w.detach()
        wc = wd if wd.is_contiguous() else wd.contiguous()
        amax = None
        if not lp:
            amax = torch.zeros(1, device=w.device, dtype=torch.float32)
            _lib.check(_lib_().wdno_amax(_p(wc), wc.numel(), _p(amax), _stream()), 'amax')
        k, c, kd, kh, kw = _wdims(kind, _as5(wc))
        rows = kd * kh * kp * kw
        if pl is None:
            pl = _WPlan()
            # (pl.w: the DETACHED weight -- same storage and version counter; a weight that arrives as a view of a parameter (Burgers' Downsample
            # weight) would otherwise keep its ViewBackward node, and through it the parameter's AccumulateGrad node, alive in this cache)
            pl.w, pl.wd, pl.kind, pl.cp8, pl.kp, pl.lp = wd, wd, kind, cp8, kp, lp
            pl.hi = torch.empty((rows, cp8), device=w.device, dtype=torch.float16)
            pl.lo = None if lp else torch.empty((rows, cp8), device=w.device, dtype=torch.float16)
            pl.sc = None if lp else torch.empty(1, device=w.device, dtype=torch.float32)
            if len(_wplans) > 4096:
                _wplans.clear(); _wtables.clear()
                bump_weight_epoch(params=False)
                ver = (w._version, WEIGHT_EPOCH)
            _wplans[key] = pl
        _lib.check(_lib_().wdno_pack_split_weight(_p(wc), _p(amax), _p(pl.hi), _p(pl.lo), _p(pl.sc), k, c, kd, kh, kw, kp, cp8,
                                                  _wmode(kind), _stream()), 'pack_split_weight')
    pl.ver = ver
    pl.used = WEIGHT_EPOCH
    return pl.hi, pl.lo, pl.sc


ACT16 = os.environ.get('WDNO_ACT16', '0') == '1'      # (OFF: measured slower) single-product mode: a convolution whose only reader is a GroupNorm stores its output as bf16, and so does the data gradient
                          # whose only reader is that norm's backward (accelerate mixed-precision semantics; test knob: fp32 storage as in round 4)
ZERO_BOX = True           # structural-zero hints reach the kernels that can use them (test knob: results are bit-identical without)


class _ZeroBox(C.Structure):          # include/wdno_hip.h: wdno_zero_box
    _fields_ = [('channels', C.c_int), ('d0', C.c_int), ('h0', C.c_int), ('w0', C.c_int)]


def set_zero_box(t, box):
    """The kernel that wrote t (diffusion_core.q_sample_cond / apply_cond: the pad condition of diffusion_2d.py:1008-1033) left zeros in every
    channel < box[0] wherever frame >= box[1] or row >= box[2] or column >= box[3]: remembered on the tensor object with its version, like an
    amax record -- any later in-place change through torch voids it."""
    t._wdno_zero_box = (tuple(int(v) for v in box), t._version)
    return t


def zero_box_of(t):
    h = getattr(t, '_wdno_zero_box', None)
    return h[0] if h is not None and h[1] == t._version and ZERO_BOX else None


def carry_zero_box(dst, src):
    """dst holds the same values as src in another layout / storage (nc_to_cl, a copy into a static buffer)."""
    box = zero_box_of(src)
    return set_zero_box(dst, box) if box is not None else dst


def conv_fwd_h3(planes, shape4, w, pack, kind, bias_p, residual, ks, st, pd, kp, out=None, osp=None, ostride=(1, 1, 1), ooff=(0, 0, 0),
                amax_rec=None, zero_box=None, out16=False):
    """planes = (hi, lo, scale) of a CL tensor with logical shape4 = (N, D, H, W) and C8 channels; w raw weight;
    pack = pack_fwd / pack_dgrad. Returns y [N, OD, OH, OW, kp] fp32. With `out` ([N, YD, YH, YW, kp]) the osp output
    pixels are placed at ooff + ostride * index (parity classes of the transposed convolution)."""
    xh, xl, sx = planes
    n, d, h, ww = shape4
    cp8 = xh.shape[-1]
    wh, wl, sw = split_weight(w, kind, cp8, kp, pack)
    if osp is None:
        osp = tuple(_out_size(a, k, s_, p_) for a, k, s_, p_ in zip((d, h, ww), ks, st, pd))
    out16 = bool(out16 and xl is None and out is None and residual is None)      # bf16 storage of y: single-product mode only
    if out is None:
        y = torch.empty((n, *osp, kp), device=xh.device, dtype=torch.bfloat16 if out16 else torch.float32)
        g = _geom((n, d, h, ww), cp8, kp, ks, st, pd, osp)
    else:
        y = out
        g = _geom((n, d, h, ww), cp8, kp, ks, st, pd, osp, y_sp=tuple(out.shape[1:4]), ostride=ostride, ooff=ooff)
    flops = 2.0 * n * osp[0] * osp[1] * osp[2] * kp * ks[0] * ks[1] * ks[2] * cp8
    tap = (out is None and tuple(st) == (1, 1, 1) and tuple(osp) == (d, h, ww) and max(ks) <= 8 and      # csrc/conv_h3t.hip: wdno_conv_h3t_takes
           ((ks[2] == 3 and cp8 % 32 == 0) or (ks[2] == 7 and cp8 % 16 == 0 and kp <= 64)))
    # layers of few pixels x many channels lend the library a workspace for the partial sums of a split reduction (csrc/conv_h3t.hip)
    wsb = 0
    if xl is not None and tap and ks[2] == 3:
        key = (n, d, h, ww, cp8, kp, tuple(ks), tuple(osp))
        wsb = _split_ws_bytes.get(key)
        if wsb is None:
            wsb = _split_ws_bytes[key] = int(_lib_().wdno_conv_fwd_split_ws_bytes(C.byref(g)))
    if LAUNCH_LOG is not None:
        LAUNCH_LOG.append(('fwd', _geom_fields(g), xl is None, residual is not None, wsb))
    with _timed(_fwd_h3_kernel_name(n * osp[0] * osp[1] * osp[2], kp, ks, tap, cp8 if xl is not None else None), flops):
        zb = None
        if zero_box is not None and tap and ks[2] == 7:      # the 7-wide stem skips the reduction stages that only see the caller's zeros (csrc/conv_h3t.hip)
            zb = _ZeroBox(*zero_box)
        if xl is None:       # single bf16 plane per operand
            if zb is not None or out16:
                _lib.check(_lib_().wdno_conv_fwd_bf16_ex(_p(xh), _p(wh), _p(bias_p), _p(residual), _p(y), int(out16), _p(amax_rec), C.byref(g),
                                                         None if zb is None else C.byref(zb), _stream()), 'conv_fwd_bf16_ex')
                return y
            _lib.check(_lib_().wdno_conv_fwd_bf16(_p(xh), _p(wh), _p(bias_p), _p(residual), _p(y), _p(amax_rec), C.byref(g), _stream()), 'conv_fwd_bf16')
            return y
        if zb is not None:
            _lib.check(_lib_().wdno_conv_fwd_f16x3_zbox(_p(xh), _p(xl), _p(sx), _p(wh), _p(wl), _p(sw), _p(bias_p), _p(residual), _p(y),
                                                        _p(amax_rec), C.byref(g), C.byref(zb), _stream()), 'conv_fwd_f16x3_zbox')
            return y
        if wsb:
            ws = torch.empty(wsb // 4, device=xh.device, dtype=torch.float32)
            _lib.check(_lib_().wdno_conv_fwd_f16x3_ws(_p(xh), _p(xl), _p(sx), _p(wh), _p(wl), _p(sw), _p(bias_p), _p(residual), _p(y),
                                                      _p(amax_rec), C.byref(g), _p(ws), wsb, _stream()), 'conv_fwd_f16x3_ws')
            return y
        _lib.check(_lib_().wdno_conv_fwd_f16x3_amax(_p(xh), _p(xl), _p(sx), _p(wh), _p(wl), _p(sw), _p(bias_p), _p(residual), _p(y),
                                                    _p(amax_rec), C.byref(g), _stream()), 'conv_fwd_f16x3')
    return y


_split_ws_bytes = {}


_pixel_tables = {}


LAUNCH_LOG = None         # tests set this to a list: ('fwd' | 'wgrad', geometry fields, ...) of every split-kernel launch below, for the plan queries


def _geom_fields(g):
    return tuple(getattr(g, k) for k, _ in _lib.ConvGeom._fields_)


def conv_fwd_plan(g, lowp=False, residual_is_y=False, split_ws_bytes=0):
    """What wdno_conv_fwd_f16x3* / _bf16* would launch for geometry g (lowp None: what wdno_conv_fwd would), as the library's own
    launch path decides it: _lib.ConvPlan (family is an index into _lib.CONV_FAMILIES). residual_is_y: the residual would be y itself.
    No launch, no device needed."""
    pl = _lib.ConvPlan()
    _lib.check(_lib_().wdno_conv_fwd_plan(C.byref(g), -1 if lowp is None else int(bool(lowp)), int(bool(residual_is_y)), int(split_ws_bytes),
                                          C.byref(pl)), 'conv_fwd_plan')
    return pl


def conv_wgrad_plan(g, lowp=False, kn=0, cn=0):
    """Same for the weight gradient (wdno_conv_wgrad_f16x3_param / _partials / _bf16_param with the parameter extents kn, cn): _lib.ConvWgradPlan."""
    pl = _lib.ConvWgradPlan()
    _lib.check(_lib_().wdno_conv_wgrad_plan(C.byref(g), int(bool(lowp)), int(kn), int(cn), C.byref(pl)), 'conv_wgrad_plan')
    return pl


def _fwd_h3_kernel_name(pixels, k, ks, tap=False, c=None):
    """Kernel family wdno_conv_fwd_f16x3 picks (mirrors the dispatch in csrc/conv_h3.hip; used as the profiling key)."""
    cdiv = lambda a, b: -(-a // b)
    tiles = cdiv(pixels, 128) * cdiv(k, 128) if k > 64 else cdiv(pixels, 256)
    small_tap = tap and ks[2] == 3 and cdiv(pixels, 64) * cdiv(k, 64) >= 64      # csrc/conv_h3.hip: the tap-resident kernel's 64-row / 128 x 64 tiles
    if (tiles >= 100 or small_tap) and max(ks) <= 8:
        cus = 256                                    # the tile shape is chosen for the device's CU count (csrc/conv_h3d.hip)
        cost = lambda bm, bn, wgt: cdiv(cdiv(pixels, bm) * cdiv(k, bn), cus) * bm * bn * wgt
        shapes = [(256, 64, 1.04), (192, 64, 1.08)] if k <= 64 else [(128, 128, 1.0), (192, 128, 1.0), (256, 64, 1.04), (192, 64, 1.08)]
        best = shapes[0]
        for sh in shapes[1:]:
            if cost(*sh) < cost(*best):
                best = sh
        if tap and ks[2] == 3:                       # csrc/conv_h3d.hip: two more shapes for the tap-resident kernel
            c_best = cost(*best)
            if k > 64 and cost(160, 128, 1.02) < c_best:
                best, c_best = (160, 128, 1.02), cost(160, 128, 1.02)
            if cost(320, 64, 1.05) < c_best:
                best, c_best = (320, 64, 1.05), cost(320, 64, 1.05)
            if cost(128, 64, 1.15) < c_best:
                best, c_best = (128, 64, 1.15), cost(128, 64, 1.15)
            if cost(64, 64, 1.35) < c_best:
                best = (64, 64, 1.35)
            # csrc/conv_h3t.hip wdno_conv_h3t_split: a long reduction on 64 x 64 tiles -> 128 x 128 tiles, the reduction cut into 4 runs
            if best[:2] == (64, 64) and c is not None and c % 32 == 0 and k >= 128:
                t128, nst = cdiv(pixels, 128) * cdiv(k, 128), ks[0] * ks[1] * (c // 32)
                if t128 * 4 <= cus and nst % 4 == 0 and nst // 4 >= 8:
                    return 'conv_fwd_h3t_kernel<128,128>/4'
        if tap and _lp() and k > 64 and cdiv(pixels, 256) * cdiv(k, 128) >= 2 * cus:
            best = (256, 128)                        # csrc/conv_h3t.hip: the wide tiles of the single-plane mode
        if tap and ks[2] == 7:
            best = (256, 64)                         # ... and the 16-channel-block kernel of 7-wide taps
            if not _lp() and cdiv(pixels, 256) < cus and cdiv(pixels, 256) < cdiv(pixels, 192) <= cus:
                best = (192, 64)                     # (less than one round of 256-pixel tiles: csrc/conv_h3t.hip)
        return f'conv_fwd_h3{"t" if tap else "d"}_kernel<{best[0]},{best[1]}>'
    return 'conv_fwd_h3_kernel<..,128>' if k > 64 else 'conv_fwd_h3_kernel<..,64>'


def _wgrad_h3_kernel_name(k, run, window=False):
    """Same for wdno_conv_wgrad_f16x3 (run = kw * C8; window: the geometries of csrc/conv_wgrad_h3d.hip's wd_window_takes)."""
    if window == 'stem':
        return 'conv_wgrad_h3s_kernel<64,352>'
    if window:
        return 'conv_wgrad_h3w_kernel<64,384>'
    cdiv = lambda a, b: -(-a // b)
    bn = 192 if cdiv(run, 192) * 192 <= cdiv(run, 128) * 128 else 128
    return f'conv_wgrad_h3d_kernel<{128 if k > 64 else 64},{bn}>'


FLAT_WGRAD = True         # weight gradients of split convolutions land in the trainer's flat gradient buffer (no gather copy for them)
_FLAT_ARMED = False       # ... only inside flat_wgrad_scope(): the trainers wrap THEIR backward in it
DEFER_WGRAD_REDUCE = True  # ... and their split reductions are collected and run as ONE launch at the end of that backward (test knob: bit-identical without)
_WGRAD_PENDING = None     # [(item, workspace), ...] while a trainer's backward is running. NOT the destination tensor: autograd's AccumulateGrad
#                           steals a gradient only when nobody else references it, and CLONES it otherwise -- a clone of a still unwritten tensor
WGRAD_FLUSH_BYTES = int(os.environ.get('WDNO_WGRAD_FLUSH_MB', '0')) << 20      # 0: one flush when the backward has returned (measured best, see conv_wgrad_h3)
DEFER_ROW_SUMS = True      # ... and so are the row sums that end a backward pass (bias gradients from column-sum partials, GroupNorm d(gamma) / d(beta)): rows_sum_for_param
_ROWSUM_PENDING = []      # [(RowsSumItem, keep-alive of the partial matrix), ...] -- filled only while _WGRAD_PENDING is a list
_DEFERRED_DSTS = set()    # flat-buffer addresses the flushed reductions wrote to (FlatBuffers.gather_grads checks that autograd kept those views)


def flush_wgrad_reduces():
    """The ordered split reductions of every weight gradient whose partial sums are waiting (conv_wgrad_h3 inside flat_wgrad_scope), in one launch
    of wdno_wgrad_reduce_multi. Until it has run, those gradient tensors are UNWRITTEN: the scope flushes when the backward returns, and anything that
    reads a gradient earlier (the bucket all-reduces that OverlappedAllReduce starts from gradient hooks) calls this first."""
    global _WGRAD_PENDING, _ROWSUM_PENDING
    pend, rows = _WGRAD_PENDING, _ROWSUM_PENDING
    if rows:                  # the row sums collected beside them (rows_sum_for_param): one more launch for all of them
        _ROWSUM_PENDING = []
        ritems = (_lib.RowsSumItem * len(rows))(*[it for it, _ in rows])
        _lib.check(_lib_().wdno_rows_sum_multi(C.cast(ritems, C.c_void_p), len(rows), _stream()), 'rows_sum_multi')
        _DEFERRED_DSTS.update(int(it.out) for it, _ in rows)
    if not pend:
        return
    _WGRAD_PENDING = [] if _FLAT_ARMED else None
    items = (_lib.WgradReduceItem * len(pend))(*[it for it, _ in pend])
    _lib.check(_lib_().wdno_wgrad_reduce_multi(C.cast(items, C.c_void_p), len(pend), _stream()), 'wgrad_reduce_multi')
    _DEFERRED_DSTS.update(int(it.dw) for it, _ in pend)


class _RowsJob:
    """A sum over the rows of a partial matrix that is still to be run: out[j] = sum_r part[r * stride + col0 + j] (csrc/pointwise.hip:
    rows_sum_multi_kernel, the fp64 sums of partial_rows_sum in the same order). `keep` holds the matrix alive."""
    __slots__ = ('keep', 'ptr', 'rows', 'stride', 'col0', 'ncols', 'is_double')

    def __init__(self, keep, ptr, rows, stride, col0, ncols, is_double):
        self.keep, self.ptr, self.rows, self.stride, self.col0, self.ncols, self.is_double = keep, ptr, rows, stride, col0, ncols, is_double

    def item(self, out, ncols=None):
        it = _lib.RowsSumItem()
        it.part, it.out, it.rows, it.stride, it.col0 = self.ptr, out.data_ptr(), self.rows, self.stride, self.col0
        it.ncols, it.is_double, it.reserved = self.ncols if ncols is None else ncols, self.is_double, 0
        return it


def rows_sum_for_param(job, param, ncols=None, out=None):
    """The gradient [ncols] of `param` from a _RowsJob. Inside a trainer's backward, when this is the parameter's first gradient since zero_grad()
    (`out` = its span of the flat gradient buffer, claimed here or by the caller): queued, run with all the others in ONE launch when the backward
    has returned (flush_wgrad_reduces) -- until then the returned view is unwritten, which is safe for the same reason as for deferred weight
    gradients (autograd only stores it). Otherwise: one launch now into a fresh tensor."""
    n = job.ncols if ncols is None else ncols
    if out is None and DEFER_ROW_SUMS and _WGRAD_PENDING is not None and param is not None:
        out = _flat_grad_out(param, (n,))
    if out is not None:
        _ROWSUM_PENDING.append((job.item(out, n), job.keep))
        return out
    dev = job.keep.device
    out = torch.empty((n,), device=dev, dtype=torch.float32)
    items = (_lib.RowsSumItem * 1)(job.item(out, n))
    _lib.check(_lib_().wdno_rows_sum_multi(C.cast(items, C.c_void_p), 1, _stream()), 'rows_sum_multi')
    return out


def take_deferred_dsts():
    """The flat-buffer addresses written by deferred reductions since the last call (trainer.FlatBuffers.gather_grads: the gradient autograd holds
    for such a parameter must BE that span -- a clone made before the reduction ran would be garbage)."""
    global _DEFERRED_DSTS
    d, _DEFERRED_DSTS = _DEFERRED_DSTS, set()
    return d


@contextlib.contextmanager
def flat_wgrad_scope():
    """Arms the direct write of weight gradients into the trainer's flat gradient buffer for the backward pass run inside this scope
    (TrainStep / TrainerCore / CapturedStep). Any other backward over a FlatBuffers-registered model -- torch.autograd.grad for a
    guidance term, a user's own loss.backward() -- allocates its gradients as usual and leaves the flat buffer alone. Inside the scope the
    split reductions of the weight gradients are deferred (flush_wgrad_reduces): one launch when the backward has returned instead of one
    behind every weight-gradient kernel."""
    global _FLAT_ARMED, _WGRAD_PENDING
    prev, _FLAT_ARMED = _FLAT_ARMED, True
    outer = _WGRAD_PENDING
    if DEFER_WGRAD_REDUCE and outer is None:
        _WGRAD_PENDING = []
    try:
        yield
    finally:
        _FLAT_ARMED = prev
        if outer is None:
            try:
                flush_wgrad_reduces()
            finally:
                _WGRAD_PENDING = None


def _flat_grad_out(w, shape):
    """The span of the trainer's flat gradient buffer that belongs to parameter w (trainer.FlatBuffers registers it), as a fresh tensor
    of `shape`, when the weight-gradient kernel may write there directly: this is the first gradient of w since zero_grad() (w.grad is
    None and no other node of this backward has claimed the span), so autograd will STORE the returned tensor -- which then already is
    the flat view gather_grads() would have copied into. None otherwise (the caller allocates)."""
    v = getattr(w, '_wdno_flat_grad', None)
    if v is None or not FLAT_WGRAD or not _FLAT_ARMED or w.grad is not None or getattr(w, '_wdno_flat_busy', True) or v.numel() != math.prod(shape) or v.device != w.device:
        return None
    w._wdno_flat_busy = True
    return v.view(shape)


def conv_wgrad_h3(xplanes, shape4, gyplanes, osp, ks, st, pd, param_kc=None, out=None):
    """-> dwp [kd, kh, K8, kw, C8] fp32 from the split planes of x (C8 channels) and dy (K8 channels); with param_kc = (K, C)
    the result comes back as [K, C, kd, kh, kw] (the parameter's layout, padding dropped) straight from the split reduction."""
    xh, xl, sx = xplanes
    gh, gl, sg = gyplanes
    n, d, h, ww = shape4
    c8, k8 = xh.shape[-1], gh.shape[-1]
    g = _geom((n, d, h, ww), c8, k8, ks, st, pd, osp)
    lib = _lib_()
    nb = lib.wdno_conv_wgrad_f16x3_ws_bytes(C.byref(g))
    ws = _ws(nb, xh.device)
    tkey = (str(xh.device), n, d, h, ww, c8, tuple(osp), tuple(ks), tuple(st), tuple(pd))
    table = _pixel_tables.get(tkey)
    if table is None:                      # geometry-only: built once, reused by every later step
        table = torch.empty((n * osp[0] * osp[1] * osp[2], 4), device=xh.device, dtype=torch.int32)
        _lib.check(lib.wdno_conv_pixel_table(_p(table), C.byref(g), _stream()), 'conv_pixel_table')
        _pixel_tables[tkey] = table
    flops = 2.0 * n * osp[0] * osp[1] * osp[2] * k8 * ks[0] * ks[1] * ks[2] * c8
    if LAUNCH_LOG is not None:
        LAUNCH_LOG.append(('wgrad', _geom_fields(g), xl is None, param_kc))
    window = tuple(st) == (1, 1, 1) and tuple(osp) == (d, h, ww) and ks[2] == 3 and pd[2] == 1 and c8 % 64 == 0
    if tuple(st) == (1, 1, 1) and tuple(osp) == (d, h, ww) and ks[2] == 7 and pd[2] == 3 and c8 == 48 and k8 <= 64 and max(ks) <= 8:
        window = 'stem'                    # csrc/conv_wgrad_h3d.hip: wd_stem_takes
    if param_kc is not None and out is not None and _WGRAD_PENDING is not None:
        # a trainer's backward and the parameter's FIRST gradient since zero_grad() (`out` is its span of the flat gradient buffer, _flat_grad_out):
        # the partial sums now, the ordered reduction with all the others when the backward has returned. Until then `out` is unwritten -- safe
        # because autograd only stores (steals) the returned view; a second gradient of the same parameter (gradient accumulation) gets out = None
        # and is reduced at once, like every weight gradient outside a trainer's backward.
        kn, cn = param_kc
        dw = out
        item = _lib.WgradReduceItem()
        with _timed(_wgrad_h3_kernel_name(k8, ks[2] * c8, window), flops):
            _lib.check(lib.wdno_conv_wgrad_partials(_p(xh), _p(xl), _p(sx), _p(gh), _p(gl), _p(sg), _p(table), _p(dw), kn, cn, _p(ws), nb, C.byref(g),
                                                    C.byref(item), _stream()), 'conv_wgrad_partials')
        _WGRAD_PENDING.append((item, ws))             # (the workspace stays alive until the flush; the destination is the trainer's buffer)
        # (A backward pass of the smoke step leaves ~400 MB of partial sums, more than the 256 MB memory-side cache: the reductions at the end read
        # them back from HBM, 2 x 127 us against 0.43 ms for the 58 launches they replace, profiles/r06_smoke_kernel_stats.md. Flushing whenever
        # ~96 MB wait keeps them cache-resident but puts five launches back between the kernels of the backward: same-box the step gained 0.07 ms
        # that way against 0.18 ms with the single flush, profiles/r06_ab_same_box.txt -- WDNO_WGRAD_FLUSH_MB stays as the knob, off.)
        if WGRAD_FLUSH_BYTES and sum(w.numel() for _, w in _WGRAD_PENDING) > WGRAD_FLUSH_BYTES:
            flush_wgrad_reduces()
        return dw
    if xl is None:           # single bf16 plane per operand
        assert param_kc is not None
        kn, cn = param_kc
        dw = out if out is not None else torch.empty((kn, cn, *ks), device=xh.device, dtype=torch.float32)
        with _timed(_wgrad_h3_kernel_name(k8, ks[2] * c8, window), flops):
            _lib.check(lib.wdno_conv_wgrad_bf16_param(_p(xh), _p(gh), _p(table), _p(dw), kn, cn, _p(ws), nb, C.byref(g), _stream()), 'conv_wgrad_bf16_param')
        return dw
    if param_kc is not None:
        kn, cn = param_kc
        dw = out if out is not None else torch.empty((kn, cn, *ks), device=xh.device, dtype=torch.float32)
        with _timed(_wgrad_h3_kernel_name(k8, ks[2] * c8, window), flops):
            _lib.check(lib.wdno_conv_wgrad_f16x3_param(_p(xh), _p(xl), _p(sx), _p(gh), _p(gl), _p(sg), _p(table), _p(dw), kn, cn, _p(ws), nb,
                                                       C.byref(g), _stream()), 'conv_wgrad_f16x3_param')
        return dw
    dwp = torch.empty((ks[0], ks[1], k8, ks[2], c8), device=xh.device, dtype=torch.float32)
    with _timed(_wgrad_h3_kernel_name(k8, ks[2] * c8, window), flops):
        _lib.check(lib.wdno_conv_wgrad_f16x3(_p(xh), _p(xl), _p(sx), _p(gh), _p(gl), _p(sg), _p(table), _p(dwp), _p(ws), nb, C.byref(g), _stream()),
                   'conv_wgrad_f16x3')
    return dwp


def _use_h3(pixels, reduction):
    return CONV_MATH in ('f16x3', 'bf16') and pixels >= H3_MIN_PIXELS and reduction >= H3_MIN_REDUCTION


def conv_reads_planes(pixels, weight):
    """Will conv_cl on a CL tensor with `pixels` output pixels and this weight read its input as fp16 (hi, lo) planes (and never as
    fp32)? Norm layers whose output feeds only such a convolution write the planes themselves (out_planes=...)."""
    if not PLANES_FWD or CONV_MATH not in ('f16x3', 'bf16') or weight.dim() < 2:
        return False
    k, c = weight.shape[0], weight.shape[1]
    vol = 1
    for v in weight.shape[2:]:
        vol *= v
    if pixels <= LINEAR_ROWS_MAX and weight.dim() == 2:
        return False
    return pad4(c) % 8 == 0 and _use_h3(pixels, pad4(c) * vol)


POISON = os.environ.get('WDNO_POISON', '0') == '1'      # debug / CI: fp32 tensors that exist only as planes are NaN-filled, so that any
#                                                          reader outside the single-reader contract fails loudly instead of reading garbage


def _poison(t):
    if POISON:
        t.fill_(float('nan'))
    return t


def _planes_only(t, planes):
    """Mark t (allocated, never written) as existing only as planes."""
    _poison(t)
    t._wdno_planes = (planes, t._version, CONV_MATH)
    t._wdno_unwritten = True
    return t


def _out_size(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def conv_fwd_raw(x, wp, bias_p, residual, ks, st, pd, kp):
    """x CL [N,D,H,W,Cp], wp [kd,kh,Kp,kw*Cp] packed -> y CL [N,OD,OH,OW,Kp]"""
    n, d, h, w, cp = x.shape
    osp = tuple(_out_size(a, k, s, p) for a, k, s, p in zip((d, h, w), ks, st, pd))
    y = torch.empty((n, *osp, kp), device=x.device, dtype=torch.float32)
    g = _geom((n, d, h, w), cp, kp, ks, st, pd, osp)
    flops = 2.0 * n * osp[0] * osp[1] * osp[2] * kp * ks[0] * ks[1] * ks[2] * cp
    with _timed('conv_fwd_kernel<128,2,2>' if kp > 64 else 'conv_fwd_kernel<64,4,1>', flops):
        _lib.check(_lib_().wdno_conv_fwd(_p(x), _p(wp), _p(bias_p), _p(residual), _p(y), C.byref(g), _stream()), 'conv_fwd')
    return y


def conv_wgrad_raw(x, dy, ks, st, pd):
    """-> dwp [kd, kh, Kp, kw, Cp] for y = conv(x, w) with dy CL [N,OD,OH,OW,Kp]"""
    n, d, h, w, cp = x.shape
    kp = dy.shape[-1]
    osp = tuple(dy.shape[1:4])
    g = _geom((n, d, h, w), cp, kp, ks, st, pd, osp)
    lib = _lib_()
    nb = lib.wdno_conv_wgrad_ws_bytes(C.byref(g))
    ws = _ws(nb, x.device)
    dwp = torch.empty((ks[0], ks[1], kp, ks[2], cp), device=x.device, dtype=torch.float32)
    flops = 2.0 * n * osp[0] * osp[1] * osp[2] * kp * ks[0] * ks[1] * ks[2] * cp
    with _timed('conv_wgrad_kernel<128,2,2>' if kp > 64 else 'conv_wgrad_kernel<64,1,4>', flops):
        _lib.check(lib.wdno_conv_wgrad(_p(x), _p(dy), _p(dwp), _p(ws), nb, C.byref(g), _stream()), 'conv_wgrad')
    return dwp


def conv_transpose_raw(x, wt, bias_p, cout_p):
    """(1,4,4)/(1,2,2)/(0,1,1) transposed convolution as 4 parity-class stride-1 convolutions.
    x CL [N,D,H,W,Cin_p] -> y CL [N,D,2H,2W,Cout_p]"""
    n, d, h, w, cp = x.shape
    y = torch.empty((n, d, 2 * h, 2 * w, cout_p), device=x.device, dtype=torch.float32)
    lib = _lib_()
    for py in range(2):
        for px in range(2):
            g = _geom((n, d, h, w), cp, cout_p, (1, 2, 2), (1, 1, 1), (0, 1 - py, 1 - px), (d, h, w),
                      y_sp=(d, 2 * h, 2 * w), ostride=(1, 2, 2), ooff=(0, py, px))
            _lib.check(lib.wdno_conv_fwd(_p(x), _p(wt[py, px]), _p(bias_p), None, _p(y), C.byref(g), _stream()), 'conv_transpose')
    return y


def colsum(x2d):
    p, c = x2d.shape
    lib = _lib_()
    nb = lib.wdno_colsum_ws_bytes(p, c)
    ws = _ws(nb, x2d.device)
    out = torch.empty((c,), device=x2d.device, dtype=torch.float32)
    _lib.check(lib.wdno_colsum(_p(x2d), _p(out), p, c, _p(ws), nb, _stream()), 'colsum')
    return out


def _pad_vec(v, n):
    if v is None or v.shape[0] == n:
        return v
    out = v.new_zeros((n,))
    out[:v.shape[0]] = v
    return out


LINEAR_MULTI_ROWS_MAX = 256    # the grouped projections (linear_multi) still beat ~40 GEMM launches at batch 256 (Burgers bf16: 103.5 -> 102.3 ms)
LINEAR_ROWS_MAX = 64      # at most LR_MAXROWS of csrc/linear_rows.hip. Beyond ~64 rows
# (the time MLPs at batch 256) the GEMM kernels win: Burgers bf16 step 123.5 -> 119.5 ms


def _linear_rows_backward(ctx, gy):
    x, weight = ctx.saved_tensors
    _, _, _, k, c, cp, kp, has_bias, _, _, _ = ctx.meta
    gy = _chk(gy, 'grad')
    rows = x.shape[0]
    lib = _lib_()
    gx = gw = gb = None
    if ctx.needs_input_grad[0]:
        wt = _cached(weight, 'lin_t', 0, 0, lambda: weight.detach().t())          # [C, K]: the data gradient is the forward on it
        gx = torch.empty((rows, cp), device=x.device, dtype=torch.float32)
        _lib.check(lib.wdno_linear_rows_fwd(_p(gy), kp, _p(wt), k, None, _p(gx), rows, k, c, cp, _stream()), 'linear_rows_dgrad')
    if ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2]):
        gw = torch.empty((k, c), device=x.device, dtype=torch.float32)
        gb = torch.empty((k,), device=x.device, dtype=torch.float32) if has_bias else None
        _lib.check(lib.wdno_linear_rows_wgrad(_p(x), cp, _p(gy), kp, _p(gw), _p(gb), rows, c, k, _stream()), 'linear_rows_wgrad')
        gw = gw.reshape(weight.shape)
        if not ctx.needs_input_grad[1]:
            gw = None
        if not (has_bias and ctx.needs_input_grad[2]):
            gb = None
    return gx, gw, gb, None, None, None


class _Conv(torch.autograd.Function):
    """y = conv(x, weight) + bias (+ residual). weight in the reference layout [K, C, (kd,) (kh, kw)] or [K, C]."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, stride, padding, with_skip=False, grad_planes=False, to_norm=False):
        ctx.with_skip = with_skip
        ctx.to_norm = to_norm and grad_planes          # the caller's statement: y goes to a GroupNorm and nowhere else
        ctx.bias_ref = bias                            # (the parameter object: its span of a trainer's flat gradient buffer, rows_sum_for_param)
        y = _Conv._forward(ctx, x, weight, bias, residual, stride, padding)
        # grad_planes: the caller states that y goes to a GroupNorm and nowhere else; if this convolution's backward reads dy
        # only through the split kernels, the norm may deliver dy as planes (and leave the fp32 tensor unwritten)
        if grad_planes and not ctx.rows and ctx.h3 and y.dim() in (4, 5) and residual is None:
            ks, st = ctx.meta[0], ctx.meta[1]
            n_, d_, h_, w_, _ = ctx.xshape
            if not ctx.needs_input_grad[0] or (st == (1, 1, 1) and _use_h3(n_ * d_ * h_ * w_, ctx.meta[6] * ks[0] * ks[1] * ks[2])):
                y._wdno_grad_planes = True
        if with_skip:              # second output: x itself (see conv_cl_skip); its gradient is folded into the dgrad epilogue
            return y, _alias_of(x)
        return y

    @staticmethod
    def _forward(ctx, x, weight, bias, residual, stride, padding):
        xrec = _known_amax(x)
        x_in = x
        ctx.x16 = x.dtype == torch.bfloat16           # a GroupNorm's planes-only output in single-product mode: never read, its gradient is bf16 too
        if ctx.x16:
            if not (getattr(x, '_wdno_unwritten', False) and x.is_cuda):
                raise RuntimeError('wdno_amd: a bf16 tensor that is not a planes-only placeholder reached a convolution')
            x = x if x.is_contiguous() else x.contiguous()
        else:
            x = _chk(x, 'x')
        lead = None
        if x.dim() != 5:       # [P, C] rows (nn.Linear) or [N, H, W, C]
            lead = x.shape[:-1]
            x5 = x.reshape(1, 1, 1, -1, x.shape[-1]) if x.dim() != 4 else x.unsqueeze(1)
        else:
            x5 = x
        w5 = _as5(weight)
        k, c = w5.shape[0], w5.shape[1]
        cp, kp = x5.shape[-1], pad4(k)
        assert cp == pad4(c), f'channel mismatch: tensor has {cp}, weight expects {c}'
        ks = tuple(w5.shape[2:])
        if x.dim() == 2 and x.shape[0] <= LINEAR_ROWS_MAX and weight.dim() == 2 and residual is None and c % 4 == 0 and k % 4 == 0:
            # nn.Linear on a handful of rows (time-embedding MLPs): one wave per output feature on the unpacked weight
            wc = weight.detach()
            wc = wc if wc.is_contiguous() else wc.contiguous()
            rows = x.shape[0]
            y = torch.empty((rows, kp), device=x.device, dtype=torch.float32)
            _lib.check(_lib_().wdno_linear_rows_fwd(_p(x), cp, _p(wc), c, _p(None if bias is None else bias.detach()), _p(y), rows, c, k, kp,
                                                    _stream()), 'linear_rows_fwd')
            ctx.save_for_backward(x, weight)
            ctx.h3 = False
            ctx.rows = True
            ctx.meta = (ks, stride, padding, k, c, cp, kp, bias is not None, False, lead, 2)
            return y
        ctx.rows = False
        with torch.no_grad():
            bias_p = _pad_vec(bias.detach() if bias is not None else None, kp)
        res5 = None
        if residual is not None:
            residual = _chk(residual, 'residual')
            res5 = residual
        osp_ = tuple(_out_size(a, kk, s_, p_) for a, kk, s_, p_ in zip(x5.shape[1:4], ks, stride, padding))
        h3 = _use_h3(x5.shape[0] * osp_[0] * osp_[1] * osp_[2], cp * ks[0] * ks[1] * ks[2])
        if getattr(x_in, '_wdno_unwritten', False):
            hp = getattr(x_in, '_wdno_planes', None)
            if not (h3 and hp is not None and hp[1] == x_in._version and hp[2] == CONV_MATH):
                raise RuntimeError('wdno_amd: a planes-only tensor reached a convolution that reads fp32')
        if h3:
            # 7-wide stems run on the 16-channel-block tap-resident kernel (csrc/conv_h3t.hip: t_stem): planes padded to whole blocks
            # (the super-resolution model's 82 channels -> 96; the base model's 42 -> 48 already are)
            c8w = pad8(cp) + 8 if (ks[2] == 7 and kp <= 64 and tuple(stride) == (1, 1, 1) and pad8(cp) % 16) else None
            planes = split_f16_of(x_in, x5.reshape(-1, cp), xrec, c8w)
            yrec = _new_amax_record(x5.device)
            # bf16 storage of y (single-product mode): its only reader is a GroupNorm whose backward will hand dy over as planes (the same test as
            # in forward() below for _wdno_grad_planes, plus the norm's own channel conditions), so no fp32 gradient of y ever has to exist
            nx_, dx_, hx_, wx_ = x5.shape[:4]
            out16 = (ACT16 and _lp() and getattr(ctx, 'to_norm', False) and GRAD_PLANES and residual is None and x.dim() in (4, 5) and kp % 8 == 0
                     and kp // 8 <= 256 and (kp // 8) & (kp // 8 - 1) == 0
                     and (not ctx.needs_input_grad[0] or (tuple(stride) == (1, 1, 1) and _use_h3(nx_ * dx_ * hx_ * wx_, kp * ks[0] * ks[1] * ks[2]))))
            y = _leave_amax(conv_fwd_h3(planes, tuple(x5.shape[:4]), weight, pack_fwd, 'f', bias_p, res5, ks, stride, padding, kp,
                                        amax_rec=yrec, zero_box=zero_box_of(x_in) if x_in.dim() == 5 else None, out16=out16), yrec)
            ctx.save_for_backward(planes[0], planes[1], planes[2], weight)     # the split planes replace x for wgrad
        else:
            y = conv_fwd_raw(x5, pack_fwd(weight, cp, kp), bias_p, res5, ks, stride, padding, kp)
            ctx.save_for_backward(x5, weight)
        ctx.h3 = h3
        ctx.xshape = tuple(x5.shape)
        ctx.meta = (ks, stride, padding, k, c, cp, kp, bias is not None, residual is not None, lead, x.dim())
        if lead is not None:
            y = y.reshape(*lead, kp) if x.dim() != 4 else y.squeeze(1)
        return y

    @staticmethod
    def backward(ctx, gy, gskip=None):
        if ctx.rows:
            return _linear_rows_backward(ctx, gy) + (None, None, None)
        return _Conv._backward(ctx, gy, gskip) + (None, None, None)

    @staticmethod
    def _backward(ctx, gy, gskip):
        if ctx.h3:
            xh, xl, sx, weight = ctx.saved_tensors
            x5 = None
        else:
            x5, weight = ctx.saved_tensors
        ks, stride, padding, k, c, cp, kp, has_bias, has_res, lead, xdim = ctx.meta
        grec = _known_amax(gy)
        po = getattr(gy, '_wdno_planes_only', None)        # GroupNorm backward delivered dy as planes + column sums; gy itself is unwritten
        if po is not None and gy.dtype == torch.bfloat16:   # (the unwritten placeholder of a bf16-stored output)
            gy = gy if gy.is_contiguous() else gy.contiguous()
        else:
            gy = _chk(gy, 'grad')
        n, d, h, w, _ = ctx.xshape
        gyplanes = None
        gb_given = None
        if po is not None:
            if not (ctx.h3 and po[2] == gy._version and po[3] == CONV_MATH and not has_res):
                raise RuntimeError('wdno_amd: a planes-only gradient reached a convolution that cannot take it')
            gyplanes, gb_given = po[0], po[1]
        osp = tuple(_out_size(a, kk, s, p) for a, kk, s, p in zip((d, h, w), ks, stride, padding))
        gy5 = gy.reshape(n, *osp, kp)
        gx = gw = gb = gr = None
        want_gb = has_bias and ctx.needs_input_grad[2]
        will_split = (ctx.needs_input_grad[1] and ctx.h3) or (ctx.needs_input_grad[0] and stride == (1, 1, 1)
                                                              and _use_h3(n * d * h * w, kp * ks[0] * ks[1] * ks[2]))
        if po is not None:
            if not (will_split and (not ctx.needs_input_grad[0] or (stride == (1, 1, 1) and _use_h3(n * d * h * w, kp * ks[0] * ks[1] * ks[2])))):
                raise RuntimeError('wdno_amd: a planes-only gradient reached a convolution whose backward needs fp32 dy')
            if want_gb:
                gb = rows_sum_for_param(gb_given, getattr(ctx, 'bias_ref', None), k) if isinstance(gb_given, _RowsJob) else gb_given[:k].contiguous()
        elif want_gb and will_split:               # dy is split for the gradient kernels anyway: column sums from the same pass
            gyplanes, gbs = split_f16_colsum(gy5.reshape(-1, kp), grec, bias=getattr(ctx, 'bias_ref', None), k=k)
            gb = gbs[:k].contiguous()
        if ctx.needs_input_grad[0]:
            gs5 = None if gskip is None else _chk(gskip, 'skip gradient').reshape(n, d, h, w, cp)      # conv_cl_skip: + gradient over the skip
            if stride == (1, 1, 1):
                pd = tuple(kk - 1 - p for kk, p in zip(ks, padding))
                if _use_h3(n * d * h * w, kp * ks[0] * ks[1] * ks[2]):
                    # dgrad = the same kernel on dy with flipped / transposed weights; "C" role = Kp, "K" role = Cp
                    if gyplanes is None:
                        gyplanes = split_f16(gy5.reshape(-1, kp), grec)
                    drec = _new_amax_record(gy5.device)       # dx is often the dy of the next convolution (projections on a residual path)
                    gx5 = _leave_amax(conv_fwd_h3(gyplanes, tuple(gy5.shape[:4]), weight, lambda w_, c8_, k_: pack_dgrad(w_, k_, c8_), 'd', None, gs5,
                                                  ks, (1, 1, 1), pd, cp, amax_rec=drec, out16=getattr(ctx, 'x16', False) and gs5 is None), drec)
                else:
                    wd = pack_dgrad(weight, cp, kp)
                    gx5 = conv_fwd_raw(gy5, wd, None, gs5, ks, (1, 1, 1), pd, cp)
                gs5 = None                                   # folded into the epilogue of the data-gradient convolution
            elif ks == (1, 4, 4) and stride == (1, 2, 2) and padding == (0, 1, 1):
                # the data gradient of the strided Downsample convolution IS the transposed convolution of dy with the same weight read as
                # [in = K (dy channels)][out = C][1][4][4]: four parity-class launches of the split kernels on the planes of dy
                oh_, ow_ = gy5.shape[2], gy5.shape[3]
                if ctx.h3 and _use_h3(n * d * oh_ * ow_, kp * 4) and _as5(weight).is_contiguous():
                    if gyplanes is None:
                        gyplanes = split_f16(gy5.reshape(-1, kp), grec)
                    drec = _new_amax_record(gy5.device)
                    gx5 = _leave_amax(conv_transpose_h3(gyplanes, tuple(gy5.shape[:4]), _as5(weight), None, cp, amax_rec=drec), drec)
                else:
                    wt = pack_transposed(_as5(weight), kp, cp)      # "in" = K (dy channels), "out" = C
                    gx5 = conv_transpose_raw(gy5, wt, None, cp)
            elif ks == (1, 2, 2) and stride == (1, 2, 2) and padding == (0, 0, 0):
                # non-overlapping patches (Burgers Downsample2d folded into a 2x2/s2 conv): each input pixel has one tap
                if ctx.h3 and _use_h3(n * d * gy5.shape[2] * gy5.shape[3], kp) and _as5(weight).is_contiguous() and PATCH_DGRAD_H3:
                    if gyplanes is None:
                        gyplanes = split_f16(gy5.reshape(-1, kp), grec)
                    drec = _new_amax_record(gy5.device)
                    gx5 = _leave_amax(_patch2_dgrad(gy5, weight, cp, kp, gyplanes, drec), drec)
                else:
                    gx5 = _patch2_dgrad(gy5, weight, cp, kp)
            else:
                raise RuntimeError(f'wdno_amd: unsupported convolution geometry for dgrad {ks} {stride} {padding}')
            if gs5 is not None:
                gx5 = gx5 + gs5
            if getattr(ctx, 'x16', False) and gx5.dtype != torch.bfloat16:
                gx5 = gx5.to(torch.bfloat16)         # (a bf16 placeholder input whose gradient could not be written as bf16 by the kernel itself)
            gx = gx5
            if lead is not None:
                gx = gx5.reshape(*lead, cp) if xdim != 4 else gx5.squeeze(1)
        if ctx.needs_input_grad[1]:
            if ctx.h3:
                if gyplanes is None:
                    gyplanes = split_f16(gy5.reshape(-1, kp), grec)
                gw = conv_wgrad_h3((xh, xl, sx), (n, d, h, w), gyplanes, osp, ks, stride, padding, param_kc=(k, c),
                                   out=_flat_grad_out(weight, (k, c, *ks))).reshape(weight.shape)
            else:
                dwp = conv_wgrad_raw(x5, gy5, ks, stride, padding)
                gw = dwp[:, :, :k, :, :c].permute(2, 4, 0, 1, 3).reshape(weight.shape).contiguous()
        if want_gb and gb is None:
            gb = colsum(gy5.reshape(-1, kp))[:k].contiguous()
        if has_res and ctx.needs_input_grad[3]:
            gr = gy
        return gx, gw, gb, gr, None, None


def _patch2_dgrad(gy5, weight, cp, kp, gyplanes=None, amax_rec=None):
    """dgrad of a (1,2,2)/s(1,2,2)/p0 conv: four 1x1 convolutions scattered to the four pixel parities. With the planes of dy: on the
    split-fp16 kernels, the operand of tap (py, px) gathered from the weight itself (kind 'q{py}{px}', refreshed with all other operands)."""
    n, d, oh, ow, _ = gy5.shape
    w5 = _as5(weight)
    gx = torch.empty((n, d, 2 * oh, 2 * ow, cp), device=gy5.device, dtype=torch.float32)
    lib = _lib_()
    if gyplanes is not None:
        for py in range(2):
            for px in range(2):
                conv_fwd_h3(gyplanes, (n, d, oh, ow), w5, None, f'q{py}{px}', None, None, (1, 1, 1), (1, 1, 1), (0, 0, 0), cp, out=gx,
                            osp=(d, oh, ow), ostride=(1, 2, 2), ooff=(0, py, px), amax_rec=amax_rec)      # the 4 taps merge into one record
        return gx

    def build():
        wz = _padded(w5.detach(), kp, cp)           # [Kp, Cp, 1, 2, 2]
        return wz.permute(3, 4, 1, 0, 2).reshape(2, 2, cp, kp)   # [py][px][C][K]
    wq = _cached(weight, 'p2', cp, kp, build)
    for py in range(2):
        for px in range(2):
            g = _geom((n, d, oh, ow), kp, cp, (1, 1, 1), (1, 1, 1), (0, 0, 0), (d, oh, ow),
                      y_sp=(d, 2 * oh, 2 * ow), ostride=(1, 2, 2), ooff=(0, py, px))
            _lib.check(lib.wdno_conv_fwd(_p(gy5), _p(wq[py, px]), None, None, _p(gx), C.byref(g), _stream()), 'patch2_dgrad')
    return gx


def conv_cl(x, weight, bias=None, stride=1, padding=0, residual=None, with_skip=False, grad_planes=False, to_norm=False):
    """Channels-last convolution / linear layer with the reference's weight layout.

    x: [N, D, H, W, Cp] or [N, H, W, Cp] with a conv weight [K, C, (kd,) kh, kw]; any [..., Cp] with a 2-D
    (nn.Linear) or 1x1 weight. stride / padding follow torch.nn conventions for the weight's rank."""
    nd = weight.dim() - 2

    def trip(v, fill):
        if nd == 0:
            return (fill,) * 3
        v = (v,) * nd if isinstance(v, int) else tuple(v)
        return (fill,) * (3 - nd) + v
    return _Conv.apply(x, weight, bias, residual, trip(stride, 1), trip(padding, 0) if nd else (0, 0, 0), with_skip, grad_planes, to_norm)


def conv_cl_skip(x, weight, bias=None, stride=1, padding=0, grad_planes=False, to_norm=False):
    """-> (conv(x), x'): x' is x handed through the operator, for blocks whose input also feeds a skip connection
    (ResnetBlock: h = block1(x) ...; out = h + x  or  res_conv(x) + h). The gradient that comes back over x' is added in the
    epilogue of this convolution's data-gradient kernel instead of by a separate accumulation launch."""
    return conv_cl(x, weight, bias, stride, padding, None, True, grad_planes, to_norm)


class _ConvT(torch.autograd.Function):
    """nn.ConvTranspose3d(dim, dim, (1,4,4), (1,2,2), (0,1,1)) on CL tensors; weight [in, out, 1, 4, 4]."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        xrec = _known_amax(x)
        x = _chk(x, 'x')
        cin, cout = weight.shape[0], weight.shape[1]
        cin_p, cout_p = x.shape[-1], pad4(cout)
        assert cin_p == pad4(cin) and tuple(weight.shape[2:]) == (1, 4, 4)
        with torch.no_grad():
            bias_p = _pad_vec(bias.detach() if bias is not None else None, cout_p)
        n, d, h, w = x.shape[:4]
        h3 = _use_h3(n * d * h * w, 4 * cin_p) and cout_p % 8 == 0
        if h3:
            planes = split_f16(x.reshape(-1, cin_p), xrec)
            yrec = _new_amax_record(x.device)
            y = _leave_amax(conv_transpose_h3(planes, (n, d, h, w), weight, bias_p, cout_p, yrec), yrec)
            ctx.save_for_backward(weight, *planes)
        else:
            y = conv_transpose_raw(x, pack_transposed(weight, cin_p, cout_p), bias_p, cout_p)
            ctx.save_for_backward(x, weight)
        ctx.meta = (cin, cout, cin_p, cout_p, bias is not None, h3, (n, d, h, w))
        return y

    @staticmethod
    def backward(ctx, gy):
        cin, cout, cin_p, cout_p, has_bias, h3, xshape4 = ctx.meta
        grec = _known_amax(gy)
        gy = _chk(gy, 'grad')
        ks, st, pd = (1, 4, 4), (1, 2, 2), (0, 1, 1)
        gx = gw = gb = None
        if h3:
            # dx = conv_s2(dy, W) with W read as a conv weight [K' = in, C' = out, 1, 4, 4]; dW from the same two operands
            weight, xh, xl, sx = ctx.saved_tensors
            gyplanes = split_f16(gy.reshape(-1, cout_p), grec)
            gshape4 = tuple(gy.shape[:4])
            if ctx.needs_input_grad[0]:
                gx = conv_fwd_h3(gyplanes, gshape4, weight, pack_fwd, 'f', None, None, ks, st, pd, cin_p)
            if ctx.needs_input_grad[1]:
                gw = conv_wgrad_h3(gyplanes, gshape4, (xh, xl, sx), xshape4[1:], ks, st, pd, param_kc=(cin, cout),
                                   out=_flat_grad_out(weight, (cin, cout, 1, 4, 4)))                                   # [in, out, 1, 4, 4]
            if has_bias and ctx.needs_input_grad[2]:
                gb = colsum(gy.reshape(-1, cout_p))[:cout].contiguous()
            return gx, gw, gb
        x, weight = ctx.saved_tensors
        if ctx.needs_input_grad[0]:
            # dx = conv_s2(dy, W) with W read as a conv weight [K' = in, C' = out, 1, 4, 4]
            wp = pack_fwd(weight, cout_p, cin_p)
            gx = conv_fwd_raw(gy, wp, None, None, ks, st, pd, cin_p)
        if ctx.needs_input_grad[1]:
            dwp = conv_wgrad_raw(gy, x, ks, st, pd)              # [1, 4, Cin_p, 4, Cout_p]
            gw = dwp[:, :, :cin, :, :cout].permute(2, 4, 0, 1, 3).contiguous()
        if has_bias and ctx.needs_input_grad[2]:
            gb = colsum(gy.reshape(-1, cout_p))[:cout].contiguous()
        return gx, gw, gb


class _LinearItem(C.Structure):
    _fields_ = [('w', C.c_void_p), ('bias', C.c_void_p), ('K', C.c_int), ('k_start', C.c_int)]


_lin_tables = {}          # (weight / bias pointers, C) -> (device table, K list, k_start list, F)


def _linear_table(weights, biases, c):
    key = (tuple(w.data_ptr() for w in weights), tuple(0 if b is None else b.data_ptr() for b in biases), c)
    tab = _lin_tables.get(key)
    if tab is None:
        if len(_lin_tables) > 64:
            _lin_tables.clear()
        items = (_LinearItem * len(weights))()
        ks, start = [], 0
        for i, (w, b) in enumerate(zip(weights, biases)):
            items[i] = _LinearItem(w.data_ptr(), None if b is None else b.data_ptr(), w.shape[0], start)
            ks.append((w.shape[0], start))
            start += w.shape[0]
        dev = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(weights[0].device)
        tab = (dev, ks, start)
        _lin_tables[key] = tab
    return tab


class _LinearMulti(torch.autograd.Function):
    """Every ResnetBlock's scale/shift projection of the same activated time embedding in ONE launch (csrc/linear_rows.hip,
    wdno_linear_multi_*), forward and backward. Outputs are views of one buffer; the gradient buffer is handed to the consumers
    (`_wdno_grad_slot`: the GroupNorm backward writes d(scale_shift) straight into its slot), so that the backward is three launches
    -- weight / bias gradients, partial data gradients, their sum -- instead of ~5 per layer."""
    @staticmethod
    def forward(ctx, x, n, *wb):
        weights, biases = wb[:n], wb[n:]
        x = _chk(x, 'x')
        p, c = x.shape
        tab, ks, f = _linear_table(weights, biases, c)
        ybuf = torch.empty((p * f,), device=x.device, dtype=torch.float32)
        _lib.check(_lib_().wdno_linear_multi_fwd(_p(tab), len(ks), f, _p(x), _p(ybuf), p, c, _stream()), 'linear_multi_fwd')
        gbuf = torch.empty_like(ybuf)
        outs = []
        for k, start in ks:
            o = ybuf[p * start:p * (start + k)].view(p, k)
            o._wdno_grad_slot = gbuf[p * start:p * (start + k)].view(p, k)
            outs.append(o)
        ctx.save_for_backward(x, *[w for w in weights])
        ctx.meta = (tab, ks, f, p, c, [b is not None for b in biases])
        ctx.gbuf = gbuf
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gys):
        x = ctx.saved_tensors[0]
        tab, ks, f, p, c, has_bias = ctx.meta
        gbuf = ctx.gbuf
        for (k, start), g in zip(ks, gys):
            slot = gbuf[p * start:p * (start + k)].view(p, k)
            if g is None:
                slot.zero_()
            elif g.data_ptr() != slot.data_ptr() or not g.is_contiguous():
                slot.copy_(g)                      # a gradient that did not come through the slot (another consumer, an accumulated sum)
        lib = _lib_()
        n = len(ks)
        gx = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty((p, c), device=x.device, dtype=torch.float32)
            nb = lib.wdno_linear_multi_dgrad_ws_bytes(f, p, c)
            ws = _ws(nb, x.device)
            _lib.check(lib.wdno_linear_multi_dgrad(_p(tab), n, f, _p(gbuf), _p(gx), p, c, _p(ws), nb, _stream()), 'linear_multi_dgrad')
        gw = torch.empty((f, c), device=x.device, dtype=torch.float32)
        gb = torch.empty((f,), device=x.device, dtype=torch.float32)
        _lib.check(lib.wdno_linear_multi_wgrad(_p(tab), n, f, _p(x), _p(gbuf), _p(gw), _p(gb), p, c, _stream()), 'linear_multi_wgrad')
        gws = tuple(gw[start:start + k] if ctx.needs_input_grad[2 + i] else None for i, (k, start) in enumerate(ks))
        gbs = tuple(gb[start:start + k] if hb and ctx.needs_input_grad[2 + n + i] else None for i, ((k, start), hb) in enumerate(zip(ks, has_bias)))
        return (gx, None) + gws + gbs


def linear_multi(x, layers):
    """[layer(x) for layer in layers] for nn.Linear layers that all read x [P, C] (P <= LINEAR_ROWS_MAX): one launch. Returns None when the
    shapes are not the ones the grouped kernels take (the caller then projects layer by layer)."""
    if not layers or x.dim() != 2 or x.shape[0] > LINEAR_MULTI_ROWS_MAX or x.shape[1] % 4 or x.shape[1] > 512 or x.dtype != torch.float32:
        return None
    ws = [l.weight for l in layers]
    if any(w.dim() != 2 or w.shape[1] != x.shape[1] or w.shape[0] % 4 or not w.is_contiguous() or w.dtype != torch.float32 for w in ws):
        return None
    bs = [l.bias for l in layers]
    return list(_LinearMulti.apply(x, len(ws), *ws, *bs))


def conv_transpose_h3(xplanes, shape4, weight, bias_p, cout_p, amax_rec=None):
    """Parity-class form of the transposed convolution on the split-fp16 kernels: 4 launches writing interleaved outputs."""
    n, d, h, w = shape4
    y = torch.empty((n, d, 2 * h, 2 * w, cout_p), device=xplanes[0].device, dtype=torch.float32)
    for py in range(2):
        for px in range(2):
            # the packed operand of the parity class is gathered from the ConvTranspose weight itself (kind 'p{py}{px}'): it is refreshed
            # with all other operands in the two launches after an optimiser step instead of ~5 small launches per class and step
            conv_fwd_h3(xplanes, shape4, weight, pack_fwd, f'p{py}{px}', bias_p, None, (1, 2, 2), (1, 1, 1), (0, 1 - py, 1 - px),
                        cout_p, out=y, osp=(d, h, w), ostride=(1, 2, 2), ooff=(0, py, px), amax_rec=amax_rec)      # the 4 classes merge into one record
    return y


def conv_transpose_cl(x, weight, bias=None):
    return _ConvT.apply(x, weight, bias)


# ----------------------------------------------------------------------------------------------------- normalisation
def _claim_grad_slot(t):
    """The gradient hand-over slot of a tensor produced by ops.linear_multi, for its FIRST consumer only: a second consumer of the same
    tensor gets None, returns a fresh gradient, autograd adds the two and _LinearMulti.backward copies the sum into the slot."""
    slot = getattr(t, '_wdno_grad_slot', None)
    if slot is not None:
        try:
            del t._wdno_grad_slot
        except AttributeError:
            pass
    return slot


def _gn_planes_ok(c):
    """The channel counts the GroupNorm planes kernels take (csrc/norm.hip: gn_planes_ok): C / 8 a power of two <= 256."""
    c8 = c // 8
    return c % 8 == 0 and c8 <= 256 and (c8 & (c8 - 1)) == 0


class _GroupNormAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, ss, groups, act_silu, eps, out_planes=False):
        x_in = x
        x = _chk_act(x, 'x')
        x16 = int(x.dtype == torch.bfloat16)
        n, c = x.shape[0], x.shape[-1]
        s = x.numel() // (n * c)
        lib = _lib_()
        nb = lib.wdno_groupnorm_ws_bytes(n, s, c, groups)
        ws = _ws(nb, x.device)
        stats = torch.empty((lib.wdno_groupnorm_stats_floats(n, c, groups),), device=x.device, dtype=torch.float32)      # (mean, rstd) + the affine tables the backward reads
        ssc = None if ss is None else _chk(ss, 'scale_shift')
        ctx.ss_slot = _claim_grad_slot(ss) if ssc is ss else None      # (ops.linear_multi: d(scale_shift) goes straight into its buffer)
        if out_planes and CONV_MATH in ('f16x3', 'bf16') and _gn_planes_ok(c):
            nbp = lib.wdno_groupnorm_fwd_planes_ws_bytes(n, s, c, groups)
            wsp = _ws(nbp, x.device)
            hi = torch.empty((n * s, c), device=x.device, dtype=torch.float16)
            lo = brec = scale = None
            if not _lp():
                lo = torch.empty((n * s, c), device=x.device, dtype=torch.float16)
                brec = _amax_slot(x.device)
                scale = brec[1:2]
            _lib.check(lib.wdno_groupnorm_act_fwd_planes_t(_p(x), x16, _p(gamma), _p(beta), _p(ssc), _p(hi), _p(lo), _p(scale), _p(stats), _p(brec),
                                                           n, s, c, groups, float(eps), int(act_silu), _p(wsp), nbp, _stream()), 'groupnorm_fwd_planes')
            ctx.save_for_backward(x, gamma, beta, ssc, stats)
            ctx.meta = (n, s, c, groups, int(act_silu))
            ctx.epoch = _param_epoch(gamma)
            ctx.grad_planes = GRAD_PLANES and getattr(x_in, '_wdno_grad_planes', False)
            # the placeholder of the planes-only output (never written). In single-product mode it is bf16-typed: the gradient the reading
            # convolution returns for it -- read by this norm's backward and by nothing else -- is then stored as bf16 as well
            y = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16 if (x16 or (ACT16 and _lp())) else torch.float32)
            return _planes_only(y, (hi, lo, scale))
        y = torch.empty(x.shape, device=x.device, dtype=torch.float32)
        rec = _new_amax_record(x.device)
        _lib.check(lib.wdno_groupnorm_act_fwd_amax_t(_p(x), x16, _p(gamma), _p(beta), _p(ssc), _p(y), _p(stats), _p(rec), n, s, c, groups,
                                                     float(eps), int(act_silu), _p(ws), nb, _stream()), 'groupnorm_fwd')
        ctx.save_for_backward(x, gamma, beta, ssc, stats)
        ctx.meta = (n, s, c, groups, int(act_silu))
        ctx.epoch = _param_epoch(gamma)
        # the convolution that produced x takes its dy as fp16 planes (conv_cl(..., grad_planes=True)): deliver dx in that form
        ctx.grad_planes = GRAD_PLANES and getattr(x_in, '_wdno_grad_planes', False) and CONV_MATH in ('f16x3', 'bf16') and _gn_planes_ok(c)
        return _leave_amax(y, rec)

    @staticmethod
    def backward(ctx, gy):
        x, gamma, beta, ss, stats = ctx.saved_tensors
        n, s, c, groups, act_silu = ctx.meta
        # The backward kernels read the affine tables the FORWARD left in `stats` (and park their two group means beside them): gamma, beta
        # and scale_shift must be what the forward saw. Autograd's version counters guard in-place changes of the saved tensors; a write
        # through the trainers' flat parameter buffer does not bump them, the weight epoch does. (One backward of a node at a time: the
        # parked means are not safe under two concurrent backward passes of the same graph on different streams.)
        if getattr(ctx, 'epoch', None) not in (None, _param_epoch(gamma)):
            raise RuntimeError('wdno_amd GroupNorm backward: the parameters were updated (optimiser step / checkpoint load) between this forward and its backward')
        gy = _chk_act(gy, 'grad')
        x16, dy16 = int(x.dtype == torch.bfloat16), int(gy.dtype == torch.bfloat16)
        lib = _lib_()
        dgb = torch.empty((n, 2, c), device=x.device, dtype=torch.float32)
        dss = None if ss is None else (ctx.ss_slot if getattr(ctx, 'ss_slot', None) is not None else torch.empty_like(ss))
        if ctx.grad_planes and CONV_MATH in ('f16x3', 'bf16'):
            nb = lib.wdno_groupnorm_bwd_planes_ws_bytes(n, s, c, groups)
            ws = _ws(nb, x.device)
            hi = torch.empty((n * s, c), device=x.device, dtype=torch.float16)
            cs = torch.empty((c,), device=x.device, dtype=torch.float32)
            lo = rec = scale = None
            if not _lp():
                lo = torch.empty((n * s, c), device=x.device, dtype=torch.float16)
                rec = _amax_slot(x.device)
                scale = rec[1:2]
            # Inside a trainer's backward the three sums that end this backward -- the column sums of dx (the bias gradient of the convolution in
            # front) and the sums over the samples of the d(gamma) / d(beta) pieces -- wait for the launch that ends the pass (rows_sum_for_param):
            # they feed parameters only. Needs gamma's and beta's spans of the flat gradient buffer; the bias span is claimed by the convolution.
            og = ob = None
            if DEFER_ROW_SUMS and _WGRAD_PENDING is not None and n > 1:
                og = _flat_grad_out(gamma, (c,))
                ob = _flat_grad_out(beta, (c,)) if og is not None else None
                if og is not None and ob is None:
                    gamma._wdno_flat_busy = False            # (give the claim back: the single-launch tail below writes fresh tensors)
                    og = None
            if og is not None:
                off, prow = C.c_size_t(0), C.c_int(0)
                _lib.check(lib.wdno_groupnorm_bwd_planes_tail(n, s, c, groups, C.byref(off), C.byref(prow)), 'groupnorm_bwd_planes_tail')
                _lib.check(lib.wdno_groupnorm_act_bwd_planes_t(_p(x), x16, _p(gy), dy16, _p(gamma), _p(beta), _p(ss), _p(stats), _p(hi), _p(lo), _p(scale), None,
                                                               _p(dgb), None, _p(dss), _p(rec), n, s, c, groups, act_silu, _p(ws), nb, _stream()),
                           'groupnorm_bwd_planes')
                dx = _poison(torch.empty_like(x))
                dx._wdno_planes_only = ((hi, lo, scale), _RowsJob(ws, ws.data_ptr() + off.value, prow.value, c, 0, c, 1), dx._version, CONV_MATH)
                dgam = rows_sum_for_param(_RowsJob(dgb, dgb.data_ptr(), n, 2 * c, 0, c, 0), gamma, out=og)
                dbet = rows_sum_for_param(_RowsJob(dgb, dgb.data_ptr(), n, 2 * c, c, c, 0), beta, out=ob)
                return dx, dgam, dbet, dss, None, None, None, None
            red = torch.empty((2 * c,), device=x.device, dtype=torch.float32) if n > 1 else None      # sum over the samples, from the same launch
            _lib.check(lib.wdno_groupnorm_act_bwd_planes_t(_p(x), x16, _p(gy), dy16, _p(gamma), _p(beta), _p(ss), _p(stats), _p(hi), _p(lo), _p(scale), _p(cs),
                                                           _p(dgb), _p(red), _p(dss), _p(rec), n, s, c, groups, act_silu, _p(ws), nb, _stream()),
                       'groupnorm_bwd_planes')
            dx = _poison(torch.empty_like(x))     # never written: the convolution reads the planes (and fails loudly if it cannot)
            dx._wdno_planes_only = ((hi, lo, scale), cs, dx._version, CONV_MATH)
            if red is None:
                red = dgb.reshape(2 * c)
            return dx, red[:c].contiguous(), red[c:].contiguous(), dss, None, None, None, None
        if x16 or dy16:
            raise RuntimeError('wdno_amd GroupNorm backward: bf16-stored activations reach the norm only together with the planes hand-over of dx '
                               '(ops.GRAD_PLANES / CONV_MATH changed between forward and backward?)')
        nb = lib.wdno_groupnorm_ws_bytes(n, s, c, groups)
        ws = _ws(nb, x.device)
        dx = torch.empty_like(x)
        rec = _new_amax_record(x.device)          # dx is the dy of the convolution in front of this norm
        _lib.check(lib.wdno_groupnorm_act_bwd_amax(_p(x), _p(gy), _p(gamma), _p(beta), _p(ss), _p(stats), _p(dx), _p(dgb), _p(dss), _p(rec),
                                                   n, s, c, groups, act_silu, _p(ws), nb, _stream()), 'groupnorm_bwd')
        red = colsum(dgb.reshape(n, 2 * c)) if n > 1 else dgb.reshape(2 * c)
        return _leave_amax(dx, rec), red[:c].contiguous(), red[c:].contiguous(), dss, None, None, None, None


class _GroupNormActAdd(torch.autograd.Function):
    """y = act(GroupNorm(x)) + residual in one apply pass (csrc/norm.hip: gn_apply_add_planes_kernel), fp32 output with its amax record."""
    @staticmethod
    def forward(ctx, x, gamma, beta, ss, residual, groups, act_silu, eps):
        x_in = x
        x = _chk_act(x, 'x')
        x16 = int(x.dtype == torch.bfloat16)
        res = _chk(residual, 'residual')
        n, c = x.shape[0], x.shape[-1]
        s = x.numel() // (n * c)
        lib = _lib_()
        nb = lib.wdno_groupnorm_fwd_planes_ws_bytes(n, s, c, groups)
        ws = _ws(nb, x.device)
        y = torch.empty(x.shape, device=x.device, dtype=torch.float32)
        stats = torch.empty((lib.wdno_groupnorm_stats_floats(n, c, groups),), device=x.device, dtype=torch.float32)      # (mean, rstd) + the affine tables the backward reads
        ssc = None if ss is None else _chk(ss, 'scale_shift')
        ctx.ss_slot = _claim_grad_slot(ss) if ssc is ss else None      # (ops.linear_multi: d(scale_shift) goes straight into its buffer)
        yrec = _new_amax_record(x.device)
        _lib.check(lib.wdno_groupnorm_act_add_fwd_planes_t(_p(x), x16, _p(gamma), _p(beta), _p(ssc), _p(res), None, _p(y), None, None, None, _p(stats),
                                                         None, _p(yrec), n, s, c, groups, float(eps), int(act_silu), _p(ws), nb, _stream()),
                   'groupnorm_add_fwd')
        ctx.save_for_backward(x, gamma, beta, ssc, stats)
        ctx.meta = (n, s, c, groups, int(act_silu))
        ctx.epoch = _param_epoch(gamma)
        ctx.grad_planes = GRAD_PLANES and getattr(x_in, '_wdno_grad_planes', False) and CONV_MATH in ('f16x3', 'bf16') and _gn_planes_ok(c)
        return _leave_amax(y, yrec)

    @staticmethod
    def backward(ctx, gy):
        r = _GroupNormAct.backward(ctx, gy)            # d/dx, d/dgamma, d/dbeta, d/dscale_shift of the normalised branch
        return r[0], r[1], r[2], r[3], gy, None, None, None


def groupnorm_act_add(x, gamma, beta, groups, residual, scale_shift=None, act=True, eps=1e-5):
    """act(GroupNorm(x)) + residual: the tail of a ResnetBlock whose skip is the identity."""
    if not (_gn_planes_ok(x.shape[-1]) and x.shape == residual.shape):
        return add(groupnorm_act(x, gamma, beta, groups, scale_shift, act, eps), residual)
    return _GroupNormActAdd.apply(x, gamma, beta, scale_shift, residual, groups, act, eps)


def groupnorm_act(x, gamma, beta, groups, scale_shift=None, act=True, eps=1e-5, out_planes=False):
    """CL GroupNorm -> optional x*(scale+1)+shift with scale_shift [N, 2C] -> optional SiLU. out_planes: the caller states that the
    result is read by one convolution that takes fp16 planes (conv_reads_planes) and by nothing else."""
    return _GroupNormAct.apply(x, gamma, beta, scale_shift, groups, act, eps, out_planes)


def _alias_of(x):
    """The same storage as a second autograd output (skip connections that pass THROUGH an operator so that its backward receives
    the skip gradient and folds the sum into its own output pass). Producer-side hints follow the alias."""
    xs = x.view_as(x)
    for attr in ('_wdno_amax', '_wdno_planes', '_wdno_unwritten'):
        h = getattr(x, attr, None)
        if h is not None:
            try:
                setattr(xs, attr, h)
            except Exception:
                pass
    return xs


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, g, eps, with_skip, out_planes=False):
        x_in = x
        x = _chk(x, 'x')
        c = x.shape[-1]
        p = x.numel() // c
        y = torch.empty_like(x)
        gf = g.reshape(-1)
        if out_planes and CONV_MATH in ('f16x3', 'bf16') and c % 8 == 0:
            hi = torch.empty((p, c), device=x.device, dtype=torch.float16)
            lo = scale = None
            if not _lp():
                lo = torch.empty((p, c), device=x.device, dtype=torch.float16)
                scale = torch.empty((1,), device=x.device, dtype=torch.float32)
            _lib.check(_lib_().wdno_layernorm_fwd_planes(_p(x), _p(gf), _p(hi), _p(lo), _p(scale), p, c, float(eps), _stream()), 'layernorm_fwd_planes')
            ctx.save_for_backward(x, g)
            ctx.eps = eps
            y = _planes_only(y, (hi, lo, scale))
            return (y, _alias_of(x_in)) if with_skip else y
        rec = _new_amax_record(x.device)
        _lib.check(_lib_().wdno_layernorm_fwd_amax(_p(x), _p(gf), _p(y), _p(rec), p, c, float(eps), _stream()), 'layernorm_fwd')
        ctx.save_for_backward(x, g)
        ctx.eps = eps
        if with_skip:
            return _leave_amax(y, rec), _alias_of(x_in)
        return _leave_amax(y, rec)

    @staticmethod
    def backward(ctx, gy, gskip=None):
        x, g = ctx.saved_tensors
        gy = _chk(gy, 'grad')
        c = x.shape[-1]
        p = x.numel() // c
        lib = _lib_()
        nb = lib.wdno_layernorm_bwd_ws_bytes(p, c)
        ws = _ws(nb, x.device)
        dx = torch.empty_like(x)
        dg = torch.empty((c,), device=x.device, dtype=torch.float32)
        add_to = None if gskip is None else _chk(gskip, 'skip gradient')
        rec = _new_amax_record(x.device)
        _lib.check(lib.wdno_layernorm_bwd_add_amax(_p(x), _p(g.reshape(-1)), _p(gy), _p(add_to), _p(dx), _p(dg), _p(rec), p, c, float(ctx.eps),
                                                   _p(ws), nb, _stream()), 'layernorm_bwd')
        return _leave_amax(dx, rec), dg.reshape(g.shape), None, None, None


def layernorm_cl(x, g, eps=1e-5, out_planes=False):
    """Channel LayerNorm over the last (channel) axis of a CL tensor; g is the reference's [1, C, 1, 1(, 1)] gain. out_planes: see
    groupnorm_act."""
    return _LayerNorm.apply(x, g, eps, False, out_planes)


def layernorm_cl_skip(x, g, eps=1e-5, out_planes=False):
    """-> (LayerNorm(x), x'): x' is x handed through the operator, for Residual(PreNorm(fn)): fn(norm(x), residual=x'). The gradient
    that comes back over x' is added inside the LayerNorm backward kernel (dx += skip) instead of by a separate launch."""
    return _LayerNorm.apply(x, g, eps, True, out_planes)


# ----------------------------------------------------------------------------------------------------- attention
class _Attn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, bias, rot_cos, rot_sin, desc_args, scale, out_planes=False):
        qkv_in = qkv
        qkv = _chk(qkv, 'qkv')
        heads = desc_args[3]
        out = torch.empty((*qkv.shape[:-1], heads * 32), device=qkv.device, dtype=torch.float32)
        d = AttnDesc(*desc_args)
        bc = None if bias is None else _chk(bias, 'bias')
        rec = _new_amax_record(qkv.device)
        qrec_f = _known_amax(qkv_in)
        planes = None
        # planes only (fp32 `out` unwritten): up to 32 tokens always -- that backward does not read `out` -- and up to 64 (the two-tile
        # forward kernel; its backward is the thread-per-row kernel, which does) when nothing here needs a gradient (sampling)
        planes_ntok = 32 if any(ctx.needs_input_grad) else 64
        if out_planes and desc_args[2] <= planes_ntok and (_lp() or (CONV_MATH == 'f16x3' and qrec_f is not None)):
            rows = out.numel() // out.shape[-1]
            hi = torch.empty((rows, heads * 32), device=qkv.device, dtype=torch.float16)
            lo = sc = None
            if not _lp():
                lo = torch.empty((rows, heads * 32), device=qkv.device, dtype=torch.float16)
                sc = torch.empty((1,), device=qkv.device, dtype=torch.float32)
            _lib.check(_lib_().wdno_attn_fwd_planes(_p(qkv), _p(rot_cos), _p(rot_sin), _p(bc), _p(out), _p(hi), _p(lo), _p(sc), _p(rec), _p(qrec_f),
                                                    C.byref(d), float(scale), _stream()), 'attn_fwd_planes')
            planes = (hi, lo, sc)
        else:
            _lib.check(_lib_().wdno_attn_fwd_amax(_p(qkv), _p(rot_cos), _p(rot_sin), _p(bc), _p(out), _p(rec), C.byref(d), float(scale), _stream()),
                       'attn_fwd')
        ctx.save_for_backward(qkv, bc, rot_cos, rot_sin, out)
        ctx.meta = (desc_args, scale)
        # the projection that produced qkv takes its dy as planes (conv_cl(..., grad_planes=True)) and left the amax of qkv
        ctx.want_planes = GRAD_PLANES and getattr(qkv_in, '_wdno_grad_planes', False) and desc_args[2] <= 32
        ctx.qrec = qrec_f if ctx.want_planes else None
        if planes is not None:                   # out stays unwritten: the n_tok <= 32 backward forms delta = sum_j P dP itself
            return _planes_only(out, planes)
        return _leave_amax(out, rec)

    @staticmethod
    def backward(ctx, go):
        qkv, bias, rot_cos, rot_sin, fout = ctx.saved_tensors
        desc_args, scale = ctx.meta
        grec = _known_amax(go)
        go = _chk(go, 'grad')
        dqkv = torch.empty_like(qkv)
        dbias = ws = None
        nbw = 0
        d = AttnDesc(*desc_args)
        if bias is not None and ctx.needs_input_grad[1]:
            dbias = torch.empty_like(bias)            # written by the ordered sum of the per-block partials in `ws` (deterministic)
            nbw = _lib_().wdno_attn_bwd_ws_bytes(C.byref(d))
            ws = _ws(nbw, qkv.device)
        if ctx.want_planes and (_lp() or (CONV_MATH == 'f16x3' and ctx.qrec is not None and grec is not None)):
            rows, rw = qkv.numel() // qkv.shape[-1], qkv.shape[-1]
            hi = torch.empty((rows, rw), device=qkv.device, dtype=torch.float16)
            lo = sc = None
            if not _lp():
                lo = torch.empty((rows, rw), device=qkv.device, dtype=torch.float16)
                sc = torch.empty((1,), device=qkv.device, dtype=torch.float32)
            _lib.check(_lib_().wdno_attn_bwd_planes(_p(qkv), _p(rot_cos), _p(rot_sin), _p(bias), _p(fout), _p(go), _p(hi), _p(lo), _p(sc),
                                                    _p(dbias), _p(ctx.qrec), _p(grec), C.byref(d), float(scale), _p(ws), nbw, _stream()), 'attn_bwd_planes')
            _poison(dqkv)
            dqkv._wdno_planes_only = ((hi, lo, sc), None, dqkv._version, CONV_MATH)      # dqkv itself stays unwritten
            return dqkv, dbias, None, None, None, None, None
        rec = _new_amax_record(qkv.device)        # dqkv is the dy of the qkv projection
        _lib.check(_lib_().wdno_attn_bwd_amax(_p(qkv), _p(rot_cos), _p(rot_sin), _p(bias), _p(fout), _p(go), _p(dqkv), _p(dbias), _p(rec),
                                              C.byref(d), float(scale), _p(ws), nbw, _stream()), 'attn_bwd')
        return _leave_amax(dqkv, rec), dbias, None, None, None, None, None


def softmax_attention(qkv, heads, n_uo, n_ui, n_tok, so, si, st, scale, bias=None, rot=None, out_planes=False):
    """qkv rows [R, 3*heads*32] (any leading shape with R rows); unit (uo, ui), token j -> row uo*so + ui*si + j*st. Returns
    [..., heads*32] with the same leading shape (pass the CL tensor itself rather than a reshaped view: tensors and gradients
    then keep the amax records their kernels leave for the neighbouring projections)."""
    rc, rs = (None, None) if rot is None else rot
    return _Attn.apply(qkv, bias, rc, rs, (n_uo, n_ui, n_tok, heads, so, si, st), scale, out_planes)


class _LinAttn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, units, n_tok, heads, scale, out_planes=False):
        qkv_in = qkv
        qkv = _chk(qkv, 'qkv')
        hd = heads * 32
        out = torch.empty((*qkv.shape[:-1], hd), device=qkv.device, dtype=torch.float32)
        kstats = torch.empty((units, hd, 2), device=qkv.device, dtype=torch.float32)
        cx = torch.empty((units, heads, 32, 32), device=qkv.device, dtype=torch.float32)
        qrec_f = _known_amax(qkv_in)
        ctx.meta = (units, n_tok, heads, scale)
        ctx.want_planes = GRAD_PLANES and getattr(qkv_in, '_wdno_grad_planes', False)      # see _Attn
        ctx.qrec = qrec_f if ctx.want_planes else None
        if out_planes and (_lp() or (CONV_MATH == 'f16x3' and qrec_f is not None)):
            rows = out.numel() // hd
            hi = torch.empty((rows, hd), device=qkv.device, dtype=torch.float16)
            lo = sc = None
            if not _lp():
                lo = torch.empty((rows, hd), device=qkv.device, dtype=torch.float16)
                sc = torch.empty((1,), device=qkv.device, dtype=torch.float32)
            _lib.check(_lib_().wdno_linattn_fwd_planes(_p(qkv), _p(hi), _p(lo), _p(sc), _p(kstats), _p(cx), _p(qrec_f), units, n_tok, heads,
                                                       float(scale), _stream()), 'linattn_fwd_planes')
            ctx.save_for_backward(qkv, kstats, cx)
            return _planes_only(out, (hi, lo, sc))          # out stays unwritten: the backward works from ctx
        rec = _new_amax_record(qkv.device)
        _lib.check(_lib_().wdno_linattn_fwd_amax(_p(qkv), _p(out), _p(kstats), _p(cx), _p(rec), units, n_tok, heads, float(scale), _stream()),
                   'linattn_fwd')
        ctx.save_for_backward(qkv, kstats, cx)
        return _leave_amax(out, rec)

    @staticmethod
    def backward(ctx, go):
        qkv, kstats, cx = ctx.saved_tensors
        units, n_tok, heads, scale = ctx.meta
        grec = _known_amax(go)
        go = _chk(go, 'grad')
        lib = _lib_()
        nb = lib.wdno_linattn_ws_bytes(units, heads)
        ws = _ws(nb, qkv.device)
        dqkv = torch.empty_like(qkv)
        if ctx.want_planes and (_lp() or (CONV_MATH == 'f16x3' and ctx.qrec is not None and grec is not None)):
            rows, rw = qkv.numel() // qkv.shape[-1], qkv.shape[-1]
            hi = torch.empty((rows, rw), device=qkv.device, dtype=torch.float16)
            lo = drec = sc = None
            if not _lp():
                lo = torch.empty((rows, rw), device=qkv.device, dtype=torch.float16)
                drec = _amax_slot(qkv.device)
                sc = drec[1:2]
            _lib.check(lib.wdno_linattn_bwd_planes(_p(qkv), _p(go), _p(kstats), _p(cx), _p(hi), _p(lo), _p(sc), _p(ctx.qrec), _p(grec), _p(drec),
                                                   _p(ws), nb, units, n_tok, heads, float(scale), _stream()), 'linattn_bwd_planes')
            _poison(dqkv)
            dqkv._wdno_planes_only = ((hi, lo, sc), None, dqkv._version, CONV_MATH)
            return dqkv, None, None, None, None, None
        rec = _new_amax_record(qkv.device)
        _lib.check(lib.wdno_linattn_bwd_amax(_p(qkv), _p(go), _p(kstats), _p(cx), _p(dqkv), _p(rec), _p(ws), nb, units, n_tok, heads,
                                             float(scale), _stream()), 'linattn_bwd')
        return _leave_amax(dqkv, rec), None, None, None, None, None


def linear_attention(qkv, units, n_tok, heads, scale, out_planes=False):
    """qkv [units*n_tok, 3*heads*32] rows (contiguous units; any leading shape) -> [..., heads*32], same leading shape."""
    return _LinAttn.apply(qkv, units, n_tok, heads, scale, out_planes)


FUSED_TATTN = True        # the level-0 temporal attention block as one launch where the kernel takes the shape (test knob: layer by layer otherwise)
FUSED_TATTN_BWD = True    # ... with gradients too: forward + ONE backward launch (csrc/attn_fused_bwd.hip); False: a training step runs the block layer by layer
FUSED_TATTN_WIDE = True   # the blocks of the 128- / 256-channel levels as one launch when nothing needs a gradient (csrc/attn_fused_wide.hip; test knob)


WIDE_SELFCHECK = os.environ.get('WDNO_WIDE_SELFCHECK', '1') != '0'
_wide_verified = {}       # (kind, shape) -> did the first-use repeats return identical bits


def _wide_selfcheck(kind, key, y, launch, repeats=3):
    """First use of a streamed-weight attention kernel (csrc/attn_fused_wide.hip, linattn_fused_wide.hip) on a shape: the launch is repeated and
    must return the SAME BITS. Why (csrc/attn_fused.h): the natural software pipeline of these kernels showed run-to-run differences of
    ~1e-6 whenever two blocks shared a CU; the cause was not found, what ships is a serialised hand-over that has never differed (40 repeats per
    shape in tests/test_gpu_wide_repro.py). An ordering hazard that timing hides may come back under another occupancy, clock or compiler -- and
    would silently break the graph == eager and replay == replay guarantees. So the guarantee is CHECKED where it is used: on any differing bit the
    wide kernels are switched off for the process (the blocks run layer by layer, as in training) and a warning says so. Never inside a stream
    capture: a captured step is always preceded by its eager warm-up, which is where the check runs. Cost: `repeats` launches + one host sync,
    once per shape and process."""
    global FUSED_TATTN_WIDE, FUSED_LATTN_WIDE
    k = (kind,) + tuple(key)
    if not WIDE_SELFCHECK or k in _wide_verified or _CAPTURE is not None or torch.cuda.is_current_stream_capturing():
        return
    ok = True
    for _ in range(repeats):
        y2 = torch.empty_like(y)
        launch(y2, None if not AMAX_HINTS or _lp() else _amax_slot(y.device))
        if not torch.equal(y, y2):
            ok = False
            break
    _wide_verified[k] = ok
    if not ok:
        import warnings
        warnings.warn(f'wdno_amd: the streamed-weight {kind} kernel did not reproduce its own bits on shape {tuple(key)}; the attention blocks of the '
                      '128- / 256-channel levels run layer by layer for the rest of this process (ops.FUSED_TATTN_WIDE = FUSED_LATTN_WIDE = False)')
        FUSED_TATTN_WIDE = FUSED_LATTN_WIDE = False


def tattn_fused_takes(x, heads, weights):
    """Does csrc/attn_fused.hip run Residual(PreNorm(temporal attention)) on this CL tensor [B, F, H, W, C] in one launch (and, when something
    in it needs a gradient, csrc/attn_fused_bwd.hip its backward in one more)?"""
    if not (FUSED_TATTN and CONV_MATH in ('f16x3', 'bf16') and x.dim() == 5 and x.is_cuda and x.dtype == torch.float32) or getattr(x, '_wdno_unwritten', False):
        return False
    if not FUSED_TATTN_BWD and torch.is_grad_enabled() and (x.requires_grad or any(w is not None and w.requires_grad for w in weights)):
        return False
    b, f, h, w, c = x.shape
    if (f != 24 or c != 64) and torch.is_grad_enabled() and (x.requires_grad or any(w_ is not None and w_.requires_grad for w_ in weights)):
        return False                             # 48 frames (the super-resolution model), 128 / 256 channels (csrc/attn_fused_wide.hip): forward only
    if c != 64 and not FUSED_TATTN_WIDE:
        return False
    return bool(_lib_().wdno_tattn_fused_takes(c, f, heads)) and b * h * w >= 64


def _tattn_operands(w_qkv, w_out, c, hd):
    if c != 64:                     # csrc/attn_fused_wide.hip streams its operands: fragment order (one load instruction = 1 KB of contiguous memory)
        return split_weight(w_qkv, 'aq', pad8(c), 3 * hd, pack_fwd) + split_weight(w_out, 'ao', hd, pad4(c), pack_fwd)
    return split_weight(w_qkv, 'f', pad8(c), 3 * hd, pack_fwd) + split_weight(w_out, 'f', hd, pad4(c), pack_fwd)


def _in_f16x3(fn):
    """The fused attention blocks compute on the split-fp16 planes whatever the arithmetic of the convolutions around them (bf16 mode)."""
    def wrap(*a, **k):
        if CONV_MATH == 'f16x3':
            return fn(*a, **k)
        with _math('f16x3'):
            return fn(*a, **k)
    return wrap


class _TAttnFused(torch.autograd.Function):
    """y = x + to_out(attention_over_frames(LayerNorm(x))): one launch forward, one launch (+ the ordered sum of the per-block weight-gradient
    partials) backward. Nothing but x and the parameters is kept for the backward -- it recomputes the block per sequence."""

    @staticmethod
    @_in_f16x3
    def forward(ctx, x, gamma, w_qkv, w_out, bias, rc, rs, eps, heads, scale):
        x = _chk(x, 'x')
        b, f, h, w, c = x.shape
        hd = heads * 32
        wqh, wql, wqs, woh, wol, wos = _tattn_operands(w_qkv, w_out, c, hd)
        bc = None if bias is None else _chk(bias, 'bias')
        y = torch.empty_like(x)
        rec = _new_amax_record(x.device)
        # a backward will follow: the launch also records max|v| (the backward's plane scale of the attention output)
        vrec = _amax_slot(x.device) if any(ctx.needs_input_grad) else None
        flops = 2.0 * b * f * h * w * (c * 3 * hd + hd * c) + 4.0 * b * h * w * heads * f * f * 32

        def launch(y_, rec_):
            _lib.check(_lib_().wdno_tattn_fused_fwd(_p(x), _p(gamma.reshape(-1)), float(eps), _p(wqh), _p(wql), _p(wqs), _p(woh), _p(wol), _p(wos),
                                                    _p(rc), _p(rs), _p(bc), _p(y_), _p(rec_), None, _p(vrec),
                                                    b, f, h * w, c, heads, float(scale), _stream()), 'tattn_fused_fwd')
        with _timed('tattn_fused_fwd_kernel', flops):
            launch(y, rec)
        if c != 64:
            _wide_selfcheck('tattn', (b, f, h * w, c, heads), y, launch)
        ctx.save_for_backward(x, gamma, w_qkv, w_out, bc, rc, rs)
        ctx.meta = (eps, heads, scale)
        ctx.vrec = vrec
        return _leave_amax(y, rec)

    @staticmethod
    @_in_f16x3
    def backward(ctx, gy):
        x, gamma, w_qkv, w_out, bias, rc, rs = ctx.saved_tensors
        eps, heads, scale = ctx.meta
        grec = _known_amax(gy)
        gy = _chk(gy, 'grad')
        if grec is None:                     # a gradient autograd summed itself: one sweep for its maximum
            grec = tensor_amax(gy)
        b, f, h, w, c = x.shape
        hd = heads * 32
        lib = _lib_()
        wqh, wql, wqs = split_weight(w_qkv, 'f', pad8(c), 3 * hd, pack_fwd)         # the forward's operand (cached per weight epoch)
        woh, wol, wos = split_weight(w_out, 'd', pad8(c), hd, lambda w_, c8_, k_: pack_dgrad(w_, k_, c8_))      # W_out^T [hd][c]
        nb = lib.wdno_tattn_fused_bwd_ws_bytes()
        ws = _ws(nb, x.device)
        dx = torch.empty_like(x)
        grads = torch.empty((lib.wdno_tattn_fused_bwd_grads(),), device=x.device, dtype=torch.float32)
        rec = _new_amax_record(x.device)
        flops = 3.0 * (2.0 * b * f * h * w * (c * 3 * hd + hd * c)) + 12.0 * b * h * w * heads * f * f * 32
        with _timed('tattn_fused_bwd_kernel', flops):
            _lib.check(lib.wdno_tattn_fused_bwd(_p(x), _p(gy), _p(gamma.reshape(-1)), float(eps), _p(wqh), _p(wql), _p(wqs), _p(woh), _p(wol), _p(wos),
                                                _p(rc), _p(rs), _p(bias), _p(grec), _p(ctx.vrec), _p(dx), _p(rec),
                                                _p(grads), _p(ws), nb, b, f, h * w, c, heads, float(scale), _stream()), 'tattn_fused_bwd')
        n_q, n_o = 3 * hd * c, c * hd
        dwq = grads[:n_q].view(3 * hd, c)
        dwo = grads[n_q:n_q + n_o].view(c, hd)
        dg = grads[n_q + n_o:n_q + n_o + c].view(gamma.shape)
        dbias = None if bias is None else grads[n_q + n_o + c:].view(heads, f, f)
        return _leave_amax(dx, rec), dg, dwq, dwo, dbias, None, None, None, None, None


def temporal_attention_fused(x, gamma, eps, w_qkv, w_out, rot, bias, heads, scale):
    """y = x + to_out(attention_over_frames(LayerNorm(x))) for CL x [B, F, H, W, 64] in ONE launch (csrc/attn_fused.hip); the projections
    read the same packed split weight operands as the layer-by-layer path (split_weight: refreshed with all others after an optimiser step)."""
    rc, rs = (None, None) if rot is None else rot
    return _TAttnFused.apply(x, gamma, w_qkv, w_out, bias, rc, rs, eps, heads, scale)


FUSED_LATTN = True        # the 64-channel SpatialLinearAttention block as two passes + a merge (test knob: layer by layer otherwise)
FUSED_LATTN_BWD = True    # ... with gradients too (csrc/linattn_fused_bwd.hip); False: a training step runs the block layer by layer
FUSED_LATTN_WIDE = True   # the blocks of the 128- / 256-channel levels in two passes + a merge when nothing needs a gradient (csrc/linattn_fused_wide.hip; test knob)


def lattn_fused_takes(x, heads, weights):
    """Does csrc/linattn_fused.hip run Residual(PreNorm(SpatialLinearAttention)) on this CL tensor [B, F, H, W, C] (and, when something in it
    needs a gradient, csrc/linattn_fused_bwd.hip its backward)?"""
    if not (FUSED_LATTN and CONV_MATH in ('f16x3', 'bf16') and x.dim() == 5 and x.is_cuda and x.dtype == torch.float32) or getattr(x, '_wdno_unwritten', False):
        return False
    needs_grad = torch.is_grad_enabled() and (x.requires_grad or any(w is not None and w.requires_grad for w in weights))
    if not FUSED_LATTN_BWD and needs_grad:
        return False
    b, f, h, w, c = x.shape
    if c != 64 and (needs_grad or not FUSED_LATTN_WIDE):
        return False                             # 128 / 256 channels (csrc/linattn_fused_wide.hip): forward only
    return bool(_lib_().wdno_lattn_fused_takes(c, heads, h * w))


class _LAttnFused(torch.autograd.Function):
    """y = x + to_out(linear_attention(LayerNorm(x))) without the [pixels x 384] projections: two passes + a merge forward, a reduction
    pass + a merge + one pass (+ the ordered sum of the weight-gradient partials) backward. Kept for the backward: x, the parameters and a
    few KB per frame (the context and the softmax statistics of k)."""

    @staticmethod
    @_in_f16x3
    def forward(ctx, x, gamma, w_qkv, w_out, b_out, eps, heads, scale):
        x = _chk(x, 'x')
        b, f, h, w, c = x.shape
        hd = heads * 32
        lib = _lib_()
        wqh, wql, wqs, woh, wol, wos = _tattn_operands(w_qkv, w_out, c, hd)       # (fragment order at 128 / 256 channels)
        units, n = b * f, h * w
        nb = lib.wdno_lattn_fused_ws_bytes(units, n)
        ws = _ws(nb, x.device)
        y = torch.empty_like(x)
        rec = _new_amax_record(x.device)
        need = any(ctx.needs_input_grad)
        cx = torch.empty((units, heads, 32, 32), device=x.device, dtype=torch.float32) if need else None
        kst = torch.empty((units, heads, 2, 32), device=x.device, dtype=torch.float32) if need else None
        bo = None if b_out is None else _chk(b_out, 'bias')
        flops = 2.0 * units * n * (c * 3 * hd + hd * c) + 4.0 * units * n * heads * 32 * 32
        def launch(y_, rec_):
            _lib.check(lib.wdno_lattn_fused_fwd(_p(x), _p(gamma.reshape(-1)), float(eps), _p(wqh), _p(wql), _p(wqs), _p(woh), _p(wol), _p(wos),
                                                _p(bo), _p(y_), _p(rec_), _p(cx), _p(kst), _p(ws), nb, units, n, c, heads, float(scale), _stream()),
                       'lattn_fused_fwd')
        with _timed('lattn_fused_fwd_kernels', flops):
            launch(y, rec)
        if c != 64:
            _wide_selfcheck('lattn', (units, n, c, heads), y, launch)
        ctx.save_for_backward(x, gamma, w_qkv, w_out, cx, kst)
        ctx.meta = (eps, heads, scale, b_out is not None)
        return _leave_amax(y, rec)

    @staticmethod
    @_in_f16x3
    def backward(ctx, gy):
        x, gamma, w_qkv, w_out, cx, kst = ctx.saved_tensors
        eps, heads, scale, has_bias = ctx.meta
        grec = _known_amax(gy)
        gy = _chk(gy, 'grad')
        if grec is None:                     # a gradient autograd summed itself: one sweep for its maximum
            grec = tensor_amax(gy)
        b, f, h, w, c = x.shape
        hd = heads * 32
        lib = _lib_()
        wqh, wql, wqs = split_weight(w_qkv, 'f', pad8(c), 3 * hd, pack_fwd)
        woh, wol, wos = split_weight(w_out, 'd', pad8(c), hd, lambda w_, c8_, k_: pack_dgrad(w_, k_, c8_))      # W_out^T [hd][c]
        units, n = b * f, h * w
        nb = lib.wdno_lattn_fused_bwd_ws_bytes(units, n)
        ws = _ws(nb, x.device)
        dx = torch.empty_like(x)
        grads = torch.empty((lib.wdno_lattn_fused_bwd_grads(),), device=x.device, dtype=torch.float32)
        rec = _new_amax_record(x.device)
        flops = 3.0 * (2.0 * units * n * (c * 3 * hd + hd * c)) + 20.0 * units * n * heads * 32 * 32
        with _timed('lattn_fused_bwd_kernels', flops):
            _lib.check(lib.wdno_lattn_fused_bwd(_p(x), _p(gy), _p(gamma.reshape(-1)), float(eps), _p(wqh), _p(wql), _p(wqs), _p(woh), _p(wol), _p(wos),
                                                _p(cx), _p(kst), _p(grec), _p(dx), _p(rec), _p(grads), _p(ws), nb, units, n, c, heads, float(scale),
                                                _stream()), 'lattn_fused_bwd')
        n_q, n_o = 3 * hd * c, c * hd
        dwq = grads[:n_q].view(w_qkv.shape)
        dwo = grads[n_q:n_q + n_o].view(w_out.shape)
        dg = grads[n_q + n_o:n_q + n_o + c].view(gamma.shape)
        dbo = grads[n_q + n_o + c:n_q + n_o + 2 * c] if has_bias else None
        return _leave_amax(dx, rec), dg, dwq, dwo, dbo, None, None, None


def linear_attention_fused(x, gamma, eps, w_qkv, w_out, b_out, heads, scale):
    """y = x + to_out(linear_attention(LayerNorm(x))) for CL x [B, F, H, W, 64] (csrc/linattn_fused.hip, csrc/linattn_fused_bwd.hip)."""
    return _LAttnFused.apply(x, gamma, w_qkv, w_out, b_out, eps, heads, scale)


def tattn_fused_plan(c, frames, batch, hw):
    """The grids the fused temporal attention launches for CL [batch, frames, H, W, c] with hw = H W, as the library's launch path decides
    them: dict(nseq, grid_fwd, grid_bwd) and, per direction d, passes_d / gstep_b_d / gstep_p_d (the walk of csrc/attn_fused.hip: sample and
    pixel steps of a block from one sequence to its next). grid_bwd = 0: no fused backward. No launch, no device needed."""
    gf, gb = C.c_int(0), C.c_int(0)
    _lib.check(_lib_().wdno_tattn_fused_plan(int(c), int(frames), int(batch), int(hw), C.byref(gf), C.byref(gb)), 'tattn_fused_plan')
    nseq = batch * hw
    out = {'nseq': nseq, 'grid_fwd': gf.value, 'grid_bwd': gb.value}
    for d, g in (('fwd', gf.value), ('bwd', gb.value)):
        if g:
            out.update({'passes_' + d: -(-nseq // g), 'gstep_b_' + d: g // hw, 'gstep_p_' + d: g % hw})
    return out


def lattn_fused_plan(units, n_tok):
    """The cuts the fused linear attention makes for `units` frames of n_tok tokens (csrc/linattn_fused.hip, linattn_fused_bwd.hip):
    dict(ntiles, chunks, tiles_per_chunk, chunks2, tiles_per_chunk2, grid2). No launch, no device needed."""
    v = [C.c_int(0) for _ in range(5)]
    _lib.check(_lib_().wdno_lattn_fused_plan(int(units), int(n_tok), *[C.byref(t) for t in v]), 'lattn_fused_plan')
    out = dict(zip(('chunks', 'tiles_per_chunk', 'chunks2', 'tiles_per_chunk2', 'grid2'), (t.value for t in v)))
    out['ntiles'] = (n_tok + 31) // 32
    return out


def _plan_dict(pl):
    return {k: getattr(pl, k) for k, _ in pl._fields_}


def attn_plan(direction, heads, n_uo, n_ui, n_tok, so=0, si=0, st=1, rot=False, bias=False, dbias=False, planes=False):
    """What softmax_attention launches forward (direction 'fwd') or backward ('bwd') for a unit / token layout, as the library's launch path
    decides it under the current debug mode: the fields of _lib.AttnPlan as a dict, `family` as a name of _lib.ATTN_FAMILIES (None when the
    call would be refused; `rc` is the code it would return). No launch, no device needed."""
    pl = _lib.AttnPlan()
    d = AttnDesc(n_uo, n_ui, n_tok, heads, so, si, st)
    fn = {'fwd': _lib_().wdno_attn_fwd_plan, 'bwd': _lib_().wdno_attn_bwd_plan}[direction]
    _lib.check(fn(C.byref(d), int(bool(rot)), int(bool(bias)), int(bool(dbias)), int(bool(planes)), C.byref(pl)), 'attn_plan')
    out = _plan_dict(pl)
    out['family'] = _lib.ATTN_FAMILIES[pl.family] if pl.family >= 0 else None
    return out


def linattn_plan(units, n_tok, heads, backward=False, ws_bytes=None):
    """The cuts linear_attention makes (csrc/linattn.hip): dict(kstats_chunks, ctx_chunks, token_tiles, family 'mfma' | 'tokens', rc).
    ws_bytes None: the workspace the backward asks for. No launch, no device needed."""
    pl = _lib.LinAttnPlan()
    if ws_bytes is None:
        ws_bytes = _lib_().wdno_linattn_ws_bytes(int(units), int(heads))
    _lib.check(_lib_().wdno_linattn_plan(int(units), int(n_tok), int(heads), int(bool(backward)), int(ws_bytes), C.byref(pl)), 'linattn_plan')
    out = _plan_dict(pl)
    out['family'] = ('mfma', 'tokens')[pl.family]
    return out


def layernorm_plan(p, c):
    """The launch shape of layernorm_cl for p rows of c channels: dict(tpr, vpl, rows_per_block, blocks, max_rows_walk, rc)."""
    pl = _lib.LayerNormPlan()
    _lib.check(_lib_().wdno_layernorm_plan(int(p), int(c), C.byref(pl)), 'layernorm_plan')
    return _plan_dict(pl)


class _RelPosBias(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight, bucket):
        w = _chk(weight, 'relative_attention_bias.weight')
        n, heads = bucket.shape[0], w.shape[1]
        out = torch.empty((heads, n, n), device=w.device, dtype=torch.float32)
        _lib.check(_lib_().wdno_relpos_bias_fwd(_p(w), _p(bucket), _p(out), n, heads, _stream()), 'relpos_bias_fwd')
        ctx.save_for_backward(bucket)
        ctx.meta = (n, heads, w.shape[0])
        return out

    @staticmethod
    def backward(ctx, g):
        (bucket,) = ctx.saved_tensors
        n, heads, nb = ctx.meta
        g = _chk(g, 'grad')
        dw = torch.empty((nb, heads), device=g.device, dtype=torch.float32)
        _lib.check(_lib_().wdno_relpos_bias_bwd(_p(g), _p(bucket), _p(dw), n, heads, nb, _stream()), 'relpos_bias_bwd')
        return dw, None


def relpos_bias(weight, bucket):
    """[heads, n, n] bias from the bucket table (conv3d.py:106-112); one launch forward, one backward."""
    return _RelPosBias.apply(weight, bucket.contiguous())


_rot_cache = {}


def rotary_tables(freqs, n):
    """cos/sin tables [n, 32] for interleaved-pair rotary embedding (rotary_embedding_torch semantics)."""
    key = (freqs.data_ptr(), freqs._version, n, str(freqs.device))
    hit = _rot_cache.get(key)
    if hit is None:
        with torch.no_grad():
            ang = (torch.arange(n, device=freqs.device, dtype=freqs.dtype)[:, None] * freqs[None, :]).repeat_interleave(2, dim=-1)
            hit = (ang.cos().contiguous(), ang.sin().contiguous())
        _rot_cache.clear()
        _rot_cache[key] = hit + (freqs.detach(),)
    return hit[0], hit[1]


# ----------------------------------------------------------------------------------------------------- wavelets
def _dwt_desc(nd, mode, L, n_img, in_dims, out_dims, cs):
    d = DwtDesc()
    d.nd, d.mode, d.L, d.n_img = nd, mode, L, n_img
    for i in range(3):
        d.in_dims[i] = in_dims[i]
        d.out_dims[i] = out_dims[i]
    d.cs_img, d.cs_band, d.cs0, d.cs1 = cs
    return d


def dwt_call(kind, src, dst, nd, mode, filters, n_img, in_dims, out_dims, cs):
    """kind in {'fwd','inv','fwd_adjoint','inv_adjoint'}; filters = 4*L python floats (dec_lo, dec_hi, rec_lo, rec_hi)."""
    lib = _lib_()
    L = len(filters) // 4
    d = _dwt_desc(nd, mode, L, n_img, in_dims, out_dims, cs)
    nb = lib.wdno_dwt_ws_bytes(C.byref(d))
    ws = _ws(nb, src.device)
    fl = (C.c_float * len(filters))(*filters)
    fn = getattr(lib, 'wdno_dwt_' + kind)
    _lib.check(fn(_p(src), _p(dst), C.byref(d), fl, _p(ws), nb, _stream()), 'dwt_' + kind)


def dwt_plan(kind, nd, mode, L, n_img, in_dims, out_dims, cs):
    """What dwt_call(kind, ...) launches for this descriptor (csrc/dwt.hip: wdno_dwt_plan_query; kind also 'fwd_packed'): dict(family 'per_axis' |
    'analysis' | 'analysis_packed' | 'synthesis2' | 'synthesis_fused' | 'synthesis3_stream' (None when rc != 0), variant, nh, tiles_h, tiles_t,
    blocks, lds_bytes, rc). Follows the debug mode and WDNO_DWT_LDS_KB as the launch does. No launch, no device needed."""
    d = _dwt_desc(nd, mode, L, n_img, in_dims, out_dims, cs)
    pl = _lib.DwtPlan()
    _lib.check(_lib_().wdno_dwt_plan_query(C.byref(d), _lib.DWT_ENTRIES.index(kind), C.byref(pl)), 'dwt_plan')
    out = _plan_dict(pl)
    out['family'] = _lib.DWT_FAMILIES[pl.family] if pl.family >= 0 else None
    return out


def pack_burgers_plan(nt, nx, nt_c, nx_c, pad_t, pad_x, ori_t, ori_x, has_low=True, cond_u0=True, cond_uT=True, L=10, B=1, fine_stride=None,
                      coarse_stride=None, align_mask=0):
    """What wdno_pack_burgers_state launches for these integers (csrc/pack_burgers.hip: wdno_pack_burgers_plan_query): dict(fine_vec, coarse_vec
    -- floats per load of the fine / coarse rows --, grid_x, grid_y, grid_z, lds_bytes, rc). Strides default to contiguous samples. No launch, no
    device needed."""
    pl = _lib.PackBurgersPlan()
    fs = 8 * nt * nx if fine_stride is None else fine_stride
    cs = 8 * nt_c * nx_c if coarse_stride is None else coarse_stride
    _lib.check(_lib_().wdno_pack_burgers_plan_query(int(fs), int(cs), int(B), int(nt), int(nx), int(nt_c), int(nx_c), int(pad_t), int(pad_x), int(ori_t),
                                                    int(ori_x), int(bool(has_low)), int(bool(cond_u0)), int(bool(cond_uT)), int(L),
                                                    int(align_mask) & 0xffffffff, C.byref(pl)), 'pack_burgers_plan')
    out = _plan_dict(pl)
    out.pop('reserved')
    return out


def upsample_coef_raw(x, outer, a, mid, b, c, fa, fb, fc):
    x = _chk(x, 'coef')
    out = torch.empty((outer * a * fa * mid * b * fb * c * fc,), device=x.device, dtype=torch.float32)
    _lib.check(_lib_().wdno_upsample_coef(_p(x), _p(out), outer, a, mid, b, c, fa, fb, fc, _stream()), 'upsample_coef')
    return out
