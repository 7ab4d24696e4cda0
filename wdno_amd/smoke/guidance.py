"""Guidance gradient of the smoke control task on the GPU (smoke/inference_2d.py:30-66, wavelet parametrisation).

The sampler calls `design_fn(x)` once per step (diffusion_2d.py:733-741); the reference evaluates
    x' = x * RESCALER ; state = IDWT3(unpack(x')) ; smoke_out = IDWT1(mean of the two halves of the last channel)
    J = - sum_b smoke_out[b, T-1] + w_energy * sum_b mean(state[b, 3:5]^2) + w_init * sum_b mean((state[b, 0, 0] - init_u)^2)
(the first two terms drop out when the model is conditioned on the control) and returns dJ/dx'. Here the same expression is
written on the HIP transforms, whose backward passes are the exact adjoint kernels (wdno_dwt_inv_adjoint), so the gradient
costs one synthesis and one adjoint-synthesis launch triple per call.

SmokeGuidance      -- the same gradient from csrc/smoke_guidance.hip (include/wdno_hip.h: wdno_smoke_guidance): two launches, no unpack copy, only
                      the part of the state J reads is synthesised. `fused_step = True` lets GaussianDiffusion.sample run every guided step as
                      U-Net -> guide() -> the fused update of the unguided loop (diffusion_core.sampling_loop); guide() predicts x0 from
                      (x_t, eps) and returns eps + g(x0) s[t].
plan()             -- pure Python: the descriptor's integers, tiles, LDS and workspace bytes; needs neither the library nor a GPU.

Tile rule. Launch 1 tiles the reconstruction by (tn frames, hn rows), launch 2 the coefficient block by (kt frames, kh rows), both full
width. A synthesis tile stages tn/2 + 2 coefficient frames and hn/2 + 2 rows (halo: 2 per side per axis), an adjoint tile reads 2 kt + 4
residual frames and 2 kh + 4 rows, so small tiles repeat work; the first pair of TILES1 and of TILES2 whose buffers fit 64 KiB of LDS is taken
(the 40 x 40 state with a 34 x 34 block: (tn, hn) = (4, 8) at 47 488 B = 46.4 KiB and (kt, kh) = (2, 4) at 20 480 B = 20 KiB; on the
80 x 80 super-resolution state the synthesis tile falls back to (4, 4), the adjoint tile stays at (2, 4)).
"""
import ctypes as C

import torch

from wdno_amd import wavelets as W
from wave_trans_2d import tensor_to_coef


def _split_row(rows):
    """inference_2d.py:44-45 writes int(40/2) whatever the tensor size: the super-resolution tensors (80 x 80) split at row 20 too. Tensors
    of 20 rows or fewer (the reduced-size tests; the reference's second mean would be over nothing there: NaN) are halved instead."""
    return 20 if rows > 20 else rows // 2


def guidance_value(x, shape, ori_shape, rescaler, wave_type='bior1.3', pad_mode='zero', is_condition_control=False, w_energy=0.0, w_init=0.0,
                   init_u=None):
    """The scalar J above (differentiable w.r.t. x). x [B, F, 42, 40, 40] in rescaled (network) units; rescaler [1, 1, 42, 1, 1]."""
    xs = x * rescaler
    coef = tensor_to_coef(xs[:, :, :-2].permute(0, 2, 1, 3, 4), shape)
    rec = W.waverec3([coef[0].contiguous(), {k: v.contiguous() for k, v in coef[1].items()}], wave_type, pad_mode)
    state = rec[:, :ori_shape[0], :ori_shape[1], :ori_shape[2]].reshape(-1, 5, ori_shape[0], ori_shape[1], ori_shape[2])
    half = _split_row(xs.shape[-2])
    lo = xs[:, :shape[0], -1, :half].mean((-2, -1)).unsqueeze(1)
    hi = xs[:, :shape[0], -1, half:].mean((-2, -1)).unsqueeze(1)
    smoke_out = W.DWT1DInverse(mode=pad_mode, wave=wave_type)((lo.contiguous(), [hi.contiguous()]))[:, 0]
    g_init = (state[:, 0, 0] - init_u.to(state.device)).square().mean((-1, -2)).sum() if init_u is not None else 0.0
    if is_condition_control:
        return w_init * g_init
    g_success = smoke_out[:, ori_shape[0] - 1].sum()
    g_energy = state[:, 3:5].square().mean((1, 2, 3, 4)).sum()
    return -g_success + w_energy * g_energy + w_init * g_init


def guidance_fn(x, shape, ori_shape, rescaler, **kw):
    """dJ/d(x * RESCALER), the quantity inference_2d.guidance_fn returns (the sampler scales it, diffusion_2d.py:733-741)."""
    with torch.enable_grad():
        xs = (x.detach() * rescaler).requires_grad_(True)
        j = guidance_value(xs, shape, ori_shape, torch.ones_like(rescaler), **kw)
        return torch.autograd.grad(j, xs)[0]


# ----------------------------------------------------------------------------------------------------- closed form (no autograd)
_success_cache = {}


def _success_gradient(t_coef, t_ori, wave_type, pad_mode, device):
    """d smoke_out[T-1] / d(lo, hi): two constant vectors of length T' (the 1-D synthesis is linear), computed once."""
    key = (t_coef, t_ori, wave_type, pad_mode, str(device))
    if key not in _success_cache:
        with torch.enable_grad():
            lo = torch.zeros(1, 1, t_coef, device=device, requires_grad=True)
            hi = torch.zeros(1, 1, t_coef, device=device, requires_grad=True)
            so = W.DWT1DInverse(mode=pad_mode, wave=wave_type)((lo, [hi]))[:, 0]
            g_lo, g_hi = torch.autograd.grad(so[:, t_ori - 1].sum(), (lo, hi))
        _success_cache[key] = (g_lo.reshape(-1).contiguous(), g_hi.reshape(-1).contiguous())
    return _success_cache[key]


def guidance_fn_explicit(x, shape, ori_shape, rescaler, wave_type='bior1.3', pad_mode='zero', is_condition_control=False, w_energy=0.0,
                         w_init=0.0, init_u=None):
    """The same gradient as guidance_fn, written out: J is quadratic in the reconstructed state and linear in the smoke-out
    channel, so  dJ/dxs = unpack^T( IDWT3^T( dJ/dstate ) ) + (constant for the smoke-out channel)  with
        dJ/dstate[:, 0, 0]  = 2 w_init (state[:, 0, 0] - init_u) / (H W),      dJ/dstate[:, 3:5] = 2 w_energy state[:, 3:5] / (2 T H W).
    One synthesis launch, one adjoint-synthesis launch (wdno_dwt_inv_adjoint) and index work; no autograd tape, no host sync --
    the guided sampling step can therefore be captured in a HIP graph like the unguided one (diffusion_core._StepGraph)."""
    from wdno_amd import ops
    from wdno_amd.wavelets import MODES, _filters
    xs = (x * rescaler).contiguous()
    b, f, c, hh, ww = xs.shape
    tc, hc, wc = (int(v) for v in shape)
    to, ho, wo = (int(v) for v in ori_shape)
    # unpack: [B, F, 40, H, W] -> packed coefficients [B*5, 8, T', H', W'] (tensor_to_coef + coef_to_tensor order)
    packed = xs[:, :tc, :40, :hc, :wc].reshape(b, tc, 5, 8, hc, wc).permute(0, 2, 3, 1, 4, 5).reshape(b * 5, 8, tc, hc, wc).contiguous()
    filt, L = _filters(wave_type)
    m = MODES[pad_mode]
    sig = [2 * v if m == 0 else 2 * v - L + 2 for v in (tc, hc, wc)]
    cs = (8 * tc * hc * wc, tc * hc * wc, hc * wc, wc)
    rec = torch.empty((b * 5, *sig), device=xs.device, dtype=torch.float32)
    ops.dwt_call('inv', packed, rec, 3, m, filt, b * 5, sig, [tc, hc, wc], cs)
    state = rec.reshape(b, 5, *sig)[:, :, :to, :ho, :wo]
    drec = torch.zeros_like(rec).reshape(b, 5, *sig)
    if init_u is not None and w_init != 0.0:
        drec[:, 0, 0, :ho, :wo] = (state[:, 0, 0] - init_u.to(state.device)) * (2.0 * w_init / (ho * wo))
    if not is_condition_control and w_energy != 0.0:
        drec[:, 3:5, :to, :ho, :wo] = state[:, 3:5] * (2.0 * w_energy / (2 * to * ho * wo))
    dpacked = torch.empty_like(packed)
    ops.dwt_call('inv_adjoint', drec.reshape(b * 5, *sig), dpacked, 3, m, filt, b * 5, sig, [tc, hc, wc], cs)
    g = torch.zeros_like(xs)
    g[:, :tc, :40, :hc, :wc] = dpacked.reshape(b, 5, 8, tc, hc, wc).permute(0, 3, 1, 2, 4, 5).reshape(b, tc, 40, hc, wc)
    if not is_condition_control:
        g_lo, g_hi = _success_gradient(tc, to, wave_type, pad_mode, xs.device)
        half = _split_row(hh)                  # the reference halves the ROW axis of the smoke-out channel (x[:, :T', -1, :20])
        g[:, :tc, -1, :half, :] -= (g_lo / (half * ww)).reshape(1, tc, 1, 1)
        g[:, :tc, -1, half:, :] -= (g_hi / ((hh - half) * ww)).reshape(1, tc, 1, 1)
    return g


# ----------------------------------------------------------------------------------------------------- the guidance kernel
LDS_BUDGET = 64 * 1024          # what a launch may ask for without opting into the large-LDS mode
SUPPORTED = {('bior1.3', 'zero')}                 # the (L, mode) instance csrc/smoke_guidance.hip is built for
TILES1 = ((4, 8), (4, 4), (2, 4), (2, 2))         # (tn, hn) of the synthesis launch, in order of preference
TILES2 = ((2, 4), (2, 2), (1, 2), (1, 1))         # (kt, kh) of the adjoint launch
NCOPY = 32                                        # workgroups per sample that only take part in the shared copy


def lds1_bytes(wc, wo, tn, hn):
    """LDS of a synthesis workgroup: a staged band pair [2][KT][KH][wc], the W pass [4][KT][KH][wo], the H pass [2][KT][hn][wo]."""
    kt, kh = tn // 2 + 2, hn // 2 + 2
    return 4 * (2 * kt * kh * wc + 4 * kt * kh * wo + 2 * kt * hn * wo)


def lds2_bytes(wo, kt, kh):
    """LDS of an adjoint workgroup: the T pass [2][kt][2 kh + 4][wo] and the H pass [4][kt][kh][wo]."""
    return 4 * (2 * kt * (2 * kh + 4) * wo + 4 * kt * kh * wo)


def plan(x_shape, shape, ori_shape, wave_type='bior1.3', pad_mode='zero', is_condition_control=False):
    """Host integers of one wdno_smoke_guidance call on a contiguous x of x_shape = (B, F, C, H, W). ValueError for a (wave, mode) the kernel
    is not built for, a block larger than the tensor, a crop larger than the reconstruction, and tiles that do not fit the LDS budget."""
    from wdno_amd.filters import filter_bank
    if (wave_type, pad_mode) not in SUPPORTED:
        raise ValueError(f'smoke guidance kernel: (wave, mode) = ({wave_type!r}, {pad_mode!r}) is not built; supported: {sorted(SUPPORTED)}')
    L = len(filter_bank(wave_type)[2])
    B, F, Cc, H, W = (int(v) for v in x_shape)
    tc, hc, wc = (int(v) for v in shape)
    to, ho, wo = (int(v) for v in ori_shape)
    if Cc < 42:
        raise ValueError(f'smoke guidance: {Cc} channels; 40 coefficient channels and the two condition channels are needed')
    if not (3 <= tc <= F and 3 <= hc <= H and 3 <= wc <= W):
        raise ValueError(f'smoke guidance: coefficient block {(tc, hc, wc)} does not fit the {(F, H, W)} tensor or is shorter than the filter')
    rec = tuple(2 * v - L + 2 for v in (tc, hc, wc))
    if not all(1 <= o <= r for o, r in zip((to, ho, wo), rec)):
        raise ValueError(f'smoke guidance: field {(to, ho, wo)} is not a crop of the {rec} reconstruction')
    if B < 1 or B > 65535 or F * Cc * H * W >= 2 ** 31 or H < 2:
        raise ValueError(f'smoke guidance: tensor {tuple(x_shape)} is outside the kernel\'s 32-bit strides / grid')
    ev = lambda v: v + (v & 1)
    t1 = [(min(tn, ev(to)), min(hn, ev(ho))) for tn, hn in TILES1]
    t1 = [t for t in t1 if lds1_bytes(wc, wo, *t) <= LDS_BUDGET]
    t2 = [(min(kt, tc), min(kh, hc)) for kt, kh in TILES2]
    t2 = [t for t in t2 if lds2_bytes(wo, *t) <= LDS_BUDGET]
    if not t1 or not t2:
        raise ValueError(f'smoke guidance: the smallest tile of a {(tc, hc, wc)} block with {wo} columns does not fit {LDS_BUDGET} B of LDS')
    (tn, hn), (kt, kh) = t1[0], t2[0]
    return dict(B=B, F=F, C=Cc, H=H, W=W, sample_stride=F * Cc * H * W, frame_stride=Cc * H * W, chan_stride=H * W, row_stride=W,
                tc=tc, hc=hc, wc=wc, to=to, ho=ho, wo=wo, L=L, mode=1, half=_split_row(H), is_condition_control=int(bool(is_condition_control)),
                tn=tn, hn=hn, kt=kt, kh=kh, ncopy=NCOPY, lds1_bytes=lds1_bytes(wc, wo, tn, hn), lds2_bytes=lds2_bytes(wo, kt, kh),
                ws_bytes=4 * B * (2 * to * ho * wo + ho * wo))


class SmokeGuidance:
    """`design_fn` for GaussianDiffusion.sample on the guidance kernel: `g(x, init_u=...)` returns dJ/d(x RESCALER) like GuidanceFn does, from
    two launches. `graph_safe` and `fused_step` tell the sampler that the guided step is U-Net -> guide() -> the fused update, captured like
    the unguided one; both are False when the kernel does not take the configuration (plan() raises), and the object then answers through
    guidance_fn_explicit.

    The initial density of the fused route lives in one device buffer per (device, shape), kept for the object's lifetime:
    set_init_u(init_u, device) refills it IN PLACE, so a captured sampling step is replayed on the next batch's initial density, and
    set_init_u(None) only switches the term off. The workspaces belong to the object, one per (device, tensor shape), and are never
    replaced or freed while the object lives: a captured step of one batch size keeps a valid pointer whatever else the object is called on."""

    def __init__(self, shape, ori_shape, rescaler, is_condition_control=False, w_energy=0.0, w_init=0.0, wave_type='bior1.3', pad_mode='zero'):
        self.shape, self.ori_shape = tuple(int(v) for v in shape), tuple(int(v) for v in ori_shape)
        self.is_condition_control, self.w_energy, self.w_init = bool(is_condition_control), float(w_energy), float(w_init)
        self.wave_type, self.pad_mode = wave_type, pad_mode
        self.rescaler = torch.as_tensor(rescaler, dtype=torch.float32)
        self.init_u = None                    # the buffer guide() reads, or None: no initial-density term
        self._u_bufs = {}                     # (device, shape) -> buffer
        self._resc, self._succ, self._ws, self._desc = {}, {}, {}, {}
        try:
            tc, hc, wc = self.shape
            plan((1, tc, max(42, self.rescaler.numel()), hc, wc), self.shape, self.ori_shape, wave_type, pad_mode, is_condition_control)
            self.graph_safe = self.fused_step = True
        except ValueError:
            self.graph_safe = self.fused_step = False

    def key(self):
        """What a captured launch of this object bakes in besides its workspace (fixed per device and tensor shape, which the step graph's
        key carries): the constants and the density buffer."""
        return (self.shape, self.ori_shape, self.is_condition_control, self.w_energy, self.w_init, self.wave_type, self.pad_mode,
                None if self.init_u is None else (tuple(self.init_u.shape), str(self.init_u.device), self.init_u.data_ptr()))

    def set_init_u(self, init_u, device=None):
        """The initial density [B, ho, wo] of the fused route, copied into the object's buffer on `device` (default: init_u's own)."""
        if init_u is None:
            self.init_u = None
            return self
        to, ho, wo = self.ori_shape
        u = torch.as_tensor(init_u).detach().reshape(-1, ho, wo)
        dev = torch.device(device) if device is not None else u.device
        if dev.type == 'cuda' and dev.index is None:
            dev = torch.device('cuda', torch.cuda.current_device())
        k = (str(dev), tuple(u.shape))
        buf = self._u_bufs.get(k)
        if buf is None:
            buf = self._u_bufs[k] = torch.empty(tuple(u.shape), dtype=torch.float32, device=dev)
        buf.copy_(u)                          # same storage on every call: captured launches read the new density
        self.init_u = buf
        return self

    # ------------------------------------------------------------------ launches
    def _launch(self, x_t, inp, t, c1, c2, s_table, clip_x0, init_u):
        from wdno_amd import _lib
        from wdno_amd.filters import filter_bank
        from wdno_amd.ops import _chk, _p, _stream
        inp = _chk(inp, 'x')
        dev = inp.device
        if inp.dim() != 5:
            raise ValueError(f'SmokeGuidance: x must be [B, F, C, H, W], got {tuple(inp.shape)}')
        if x_t is not None:                   # fused mode: everything the launch indexes is checked here, a mismatch would read out of bounds
            nT = int(s_table.numel())
            if tuple(x_t.shape) != tuple(inp.shape) or x_t.device != dev:
                raise ValueError(f'SmokeGuidance.guide: x_t {tuple(x_t.shape)} on {x_t.device} against eps {tuple(inp.shape)} on {dev}')
            if t.dtype != torch.int64 or tuple(t.shape) != (inp.shape[0],) or t.device != dev or not t.is_contiguous():
                raise ValueError(f'SmokeGuidance.guide: t must be a contiguous int64 [{inp.shape[0]}] on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}')
            for name, tab in (('s_table', s_table), ('sqrt_recip_alphas_cumprod', c1), ('sqrt_recipm1_alphas_cumprod', c2)):
                if tab.dtype != torch.float32 or tab.device != dev or tab.dim() != 1 or not tab.is_contiguous() or tab.numel() < nT or nT < 1:
                    raise ValueError(f'SmokeGuidance.guide: {name} must be a contiguous fp32 table of at least {nT} entries on {dev}, '
                                     f'got {tab.dtype} {tuple(tab.shape)} on {tab.device}')
        if init_u is not None:
            if init_u.device != dev or init_u.dtype != torch.float32 or not init_u.is_contiguous():
                init_u = init_u.to(dev, torch.float32).contiguous()
            if init_u.numel() != inp.shape[0] * self.ori_shape[1] * self.ori_shape[2]:
                raise ValueError(f'SmokeGuidance: init_u {tuple(init_u.shape)} against batch {inp.shape[0]} of fields {self.ori_shape[1:]}')
        key = (tuple(inp.shape), bool(clip_x0), 0 if s_table is None else int(s_table.numel()), init_u is not None)
        d = self._desc.get(key)
        if d is None:
            pl = plan(tuple(inp.shape), self.shape, self.ori_shape, self.wave_type, self.pad_mode, self.is_condition_control)
            nws = pl.pop('ws_bytes')
            desc = _lib.SmokeGuidanceDesc(**pl, num_timesteps=key[2], clip_x0=int(bool(clip_x0)), has_init_u=int(init_u is not None),
                                          w_energy=self.w_energy, w_init=self.w_init)
            filt = [float(v) for bank in filter_bank(self.wave_type) for v in bank]
            d = self._desc[key] = (desc, (C.c_float * len(filt))(*filt), nws)
        r = self._resc.get(dev)
        if r is None:
            r = self._resc[dev] = self.rescaler.reshape(-1).to(dev).contiguous()
        if r.numel() != inp.shape[2]:
            raise ValueError(f'SmokeGuidance: RESCALER has {r.numel()} channels, x has {inp.shape[2]}')
        succ = None
        if not self.is_condition_control:
            succ = self._succ.get(dev)
            if succ is None:
                succ = self._succ[dev] = torch.stack(_success_gradient(self.shape[0], self.ori_shape[0], self.wave_type, self.pad_mode, dev)).contiguous()
        wkey = (dev, tuple(inp.shape))        # one workspace per tensor shape, never replaced: a captured step holds its raw address
        ws = self._ws.get(wkey)
        if ws is None:
            ws = self._ws[wkey] = torch.empty(max(d[2], 16), dtype=torch.uint8, device=dev)
        out = torch.empty_like(inp)
        _lib.check(_lib.load().wdno_smoke_guidance(_p(x_t), _p(inp), _p(t), _p(c1), _p(c2), _p(s_table), _p(r), _p(init_u), _p(succ), _p(out),
                                                   _p(ws), ws.numel(), C.byref(d[0]), d[1], _stream()), 'wdno_smoke_guidance')
        return out

    def __call__(self, x, low=None, init=None, init_u=None):
        """dJ/d(x RESCALER) (gradient mode); low and init are ignored, as the reference's objective ignores them."""
        if not self.graph_safe:
            return guidance_fn_explicit(x, self.shape, self.ori_shape, self.rescaler.to(x.device), self.wave_type, self.pad_mode,
                                        self.is_condition_control, self.w_energy, self.w_init, init_u)
        return self._launch(None, x.detach(), None, None, None, None, False, init_u)

    def guide(self, mod, x_t, eps, t, s_table, clip_x0):
        """One sampling step's guidance (fused mode): eps + g(x0) s_table[t] with x0 = c1[t] x_t - c2[t] eps (clamped when clip_x0), the schedule
        tables of the diffusion module `mod`, t a device int64 [B] and the initial density of set_init_u."""
        from wdno_amd.ops import _chk
        if self.init_u is not None and self.init_u.device != eps.device:
            self.set_init_u(self.init_u, eps.device)
        return self._launch(_chk(x_t, 'x_t'), eps, t, mod.sqrt_recip_alphas_cumprod, mod.sqrt_recipm1_alphas_cumprod, s_table, clip_x0, self.init_u)


class CascadeGuidance:
    """`design_fn` of the super-resolution cascade (load_model's closure, smoke/inference_2d.py:81-91): one SmokeGuidance per level -- level 0
    on the base model's 42-channel RESCALER, level i on the super model's 82-channel one with shape[i], ori_shape[i] -- behind the interface
    the sampler uses (fused_step, graph_safe, set_init_u, guide, key, __call__), so every level keeps the captured guided step.

    The reference dispatches on `low is None`; a level's tensor has its RESCALER's channel count, and its initial density its field size, so
    the object dispatches on the tensor it is given. At a super level the reference's guidance_fn calls tensor_to_coef without upsample_type
    and therefore reads the coefficient block at offset 0 of the tensor whose block sits at offset 1, and splits the smoke-out rows at
    int(40 / 2); SmokeGuidance does both already, and this object leaves it so."""

    def __init__(self, levels):
        self.levels = list(levels)
        chans = [int(g.rescaler.numel()) for g in self.levels]
        fields = [g.ori_shape[1:] for g in self.levels]
        if len(set(chans)) != len(chans) and len(set(fields)) != len(fields):
            raise ValueError(f'CascadeGuidance: levels with channels {chans} and fields {fields} cannot be told apart')
        self._active = None

    @property
    def fused_step(self):
        return all(g.fused_step for g in self.levels)

    @property
    def graph_safe(self):
        return all(g.graph_safe for g in self.levels)

    def level_of(self, x):
        """The level whose tensor x [B, F, C, H, W] is: by channel count, then by the initial density's field size set last."""
        hits = [g for g in self.levels if int(g.rescaler.numel()) == int(x.shape[2])]
        if len(hits) == 1:
            return hits[0]
        if self._active is not None and self._active in hits:
            return self._active
        raise ValueError(f'CascadeGuidance: no single level takes a tensor of {tuple(x.shape)}')

    def set_init_u(self, init_u, device=None):
        if init_u is None:
            for g in self.levels:
                g.set_init_u(None)
            self._active = None
            return self
        hw = tuple(int(v) for v in init_u.shape[-2:])
        hits = [g for g in self.levels if tuple(g.ori_shape[1:]) == hw]
        if len(hits) != 1:
            raise ValueError(f'CascadeGuidance: an initial density of {hw} cells belongs to {len(hits)} of the levels {[g.ori_shape for g in self.levels]}')
        self._active = hits[0]
        hits[0].set_init_u(init_u, device)
        return self

    def key(self):
        """The key of the level whose initial density was set last (the sampler sets it right before it builds the step's key), so one
        level's captured step does not depend on the other level's buffers."""
        if self._active is None:
            return tuple(g.key() for g in self.levels)
        return (self.levels.index(self._active), self._active.key())

    def guide(self, mod, x_t, eps, t, s_table, clip_x0):
        return self.level_of(eps).guide(mod, x_t, eps, t, s_table, clip_x0)

    def __call__(self, x, low=None, init=None, init_u=None):
        return self.level_of(x)(x, low=low, init=init, init_u=init_u)


class GuidanceFn:
    """`design_fn` for GaussianDiffusion.sample (called as design_fn(x, low=, init=, init_u=), inference_2d.py:30-66) on the explicit
    gradient. `graph_safe = True` tells the sampler that the callback launches only capturable work."""
    graph_safe = True

    def __init__(self, shape, ori_shape, rescaler, **kw):
        self.shape, self.ori_shape, self.rescaler, self.kw = shape, ori_shape, rescaler, kw

    def __call__(self, x, low=None, init=None, init_u=None):
        return guidance_fn_explicit(x, self.shape, self.ori_shape, self.rescaler, init_u=init_u, **self.kw)
