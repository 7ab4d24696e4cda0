"""The control objective of the Burgers evaluation and its gradient on the GPU (eval_ddpm_burgers.py:108-147 get_loss_fn_2dconv /
get_nablaJ_2dconv, test_util.py:100-126 ddpm_guidance_loss; wavelet parametrisation).

For a network-unit tensor x [B, C, H, W], coefficient shape `shape` = (h, w), field shape `ori_shape` = (n_t, n_x):
    coef = (x RESCALER)[:, 0:8, :h, :w] ; u_f = IDWT2(coef)[:, :, :n_t, :n_x] ; u = u_f[:, 0] ; f = u_f[:, 1, :n_t - 1]
    J    = wu (sum_b mean_x[(u[b, 0] - u_target[b, 0])^2 + (1 - condition_f) (u[b, -1] - u_target[b, -1])^2] + wf sum f^2)

guidance_value()   -- J written on wdno_amd.wavelets.DWTInverse and tensor_to_coef, differentiable: with model_utils.get_nablaJ it is the
                      reference's route (autograd through the adjoint DWT kernels) and the cross-check of the kernel.
BurgersGuidance    -- nablaJ in closed form, one launch of csrc/burgers_guidance.hip (include/wdno_hip.h: wdno_burgers_guidance). J is
                      quadratic and the synthesis linear, so no tape is needed; `graph_safe = True` lets GaussianDiffusion.sample capture
                      the guided step (diffusion_core.guided_sampling_loop_burgers), where the same launch also predicts x0 from (x_t, eps)
                      and adds g s[t] to eps.
plan()             -- pure Python: the descriptor's integers (strides, tiles, LDS bytes, the coefficient rows field u touches); needs
                      neither the library nor a GPU.

Tile rule. A sample is 1 + ntile workgroups: one for field u, ntile column tiles of field f. A tile of tw coefficient columns stages
tw + L - 2 of them, so narrow tiles repeat work and wide ones leave CUs idle: tw is the widest value <= 16 whose buffers fit 64 KiB of
LDS (the evaluation's 41 x 60 block: 4 tiles of 15 columns, 42 KB; batch 50 is then 250 workgroups on 256 CUs), re-balanced so that the
tiles are equal.
"""
import ctypes as C

import torch

from wdno_amd.filters import filter_bank

LDS_BUDGET = 64 * 1024          # what a launch may ask for without opting into the large-LDS mode
TILE_MAX = 16
SUPPORTED = {('bior2.4', 'periodization'), ('bior2.4', 'per')}     # the (L, mode) instances csrc/burgers_guidance.hip is built for


def lds_bytes(h, w, n_t, tw, L):
    """Bytes of LDS a workgroup of csrc/burgers_guidance.hip uses: the taps, then the larger of the field-f tile buffers (coefficients
    [4][h][tq], (lo_w, hi_w) [2][n_t - 1][tq], residual [n_t - 1][rw]) and the field-u row buffers."""
    tq, rw, nr = tw + L - 2, 2 * tw + L - 2, n_t - 1
    return 4 * (2 * L + max(4 * h * tq + 2 * nr * tq + nr * rw, 8 * w))


def u_rows(h, n_t, L, condition_f=False):
    """Coefficient rows k whose gradient in field u is not structurally zero: those with a tap m = (i + L/2 - 1 - 2k) mod 2h < L for a
    reconstruction row i in {0, n_t - 1} ({0} when condition_f)."""
    rows = set()
    for i in ((0,) if condition_f else (0, n_t - 1)):
        rows.update(k for k in range(h) if (i + L // 2 - 1 - 2 * k) % (2 * h) < L)
    return sorted(rows)


def plan(x_shape, shape, ori_shape, wave_type='bior2.4', pad_mode='periodization', is_super_model=False, condition_f=False):
    """Host integers of one wdno_burgers_guidance call on a contiguous x of x_shape = (B, C, H, W). ValueError for a (wave, mode) the
    kernel is not built for, for sizes it cannot take, and for a block whose narrowest tile does not fit the LDS budget."""
    if (wave_type, pad_mode) not in SUPPORTED:
        raise ValueError(f'burgers guidance kernel: (wave, mode) = ({wave_type!r}, {pad_mode!r}) is not built; supported: {sorted(SUPPORTED)}')
    L = len(filter_bank(wave_type)[2])
    B, Cc, H, W = (int(v) for v in x_shape)
    h, w = int(shape[-2]), int(shape[-1])
    n_t, n_x = int(ori_shape[-2]), int(ori_shape[-1])
    if Cc < 8 or (is_super_model and Cc < 16):
        raise ValueError(f'burgers guidance: {Cc} channels; the coefficient channels 0-7 are needed')
    if not (0 < h <= H and 0 < w <= W and 2 * h >= L and 2 * w >= L):
        raise ValueError(f'burgers guidance: coefficient block {h} x {w} does not fit the {H} x {W} tensor or is shorter than the filter')
    if not (2 <= n_t <= 2 * h and 1 <= n_x <= 2 * w):
        raise ValueError(f'burgers guidance: field {n_t} x {n_x} is not a crop of the {2 * h} x {2 * w} reconstruction')
    if B < 1 or B > 65535 or B * Cc * H * W >= 2 ** 31:
        raise ValueError(f'burgers guidance: tensor {tuple(x_shape)} is outside the kernel\'s 32-bit strides / grid')
    tw = min(TILE_MAX, w)
    while tw > 1 and lds_bytes(h, w, n_t, tw, L) > LDS_BUDGET:
        tw -= 1
    if lds_bytes(h, w, n_t, tw, L) > LDS_BUDGET:
        raise ValueError(f'burgers guidance: a one-column tile of a {h} x {w} block needs {lds_bytes(h, w, n_t, tw, L)} B of LDS (> {LDS_BUDGET})')
    ntile = -(-w // tw)
    tw = -(-w // ntile)
    return dict(B=B, C=Cc, H=H, W=W, sample_stride=Cc * H * W, chan_stride=H * W, row_stride=W, h=h, w=w, n_t=n_t, n_x=n_x, L=L, mode=0,
                ntile=ntile, tw=tw, lds_bytes=lds_bytes(h, w, n_t, tw, L), u_rows=u_rows(h, n_t, L, condition_f))


def guidance_value(x, u_target, shape, ori_shape, rescaler, wu, wf, condition_f=False, wave_type='bior2.4', pad_mode='periodization',
                   is_super_model=False):
    """The scalar J of the module docstring, differentiable with respect to x (eval_ddpm_burgers.py:122-142)."""
    from wdno_amd.wavelets import DWTInverse
    from wave_trans import tensor_to_coef
    n_t, n_x = int(ori_shape[-2]), int(ori_shape[-1])
    x = x[:, :8] * rescaler[:, :8] if is_super_model else x * rescaler
    yl, yh = tensor_to_coef(x, shape)
    u_f = DWTInverse(mode=pad_mode, wave=wave_type)((yl.contiguous(), [v.contiguous() for v in yh]))[:, :, :n_t, :n_x]
    u, f = u_f[:, 0], u_f[:, 1, :n_t - 1]
    ut = u_target[:, :n_t, :n_x]
    loss_u = (u[:, 0] - ut[:, 0]).square()
    if not condition_f:
        loss_u = loss_u + (u[:, -1] - ut[:, -1]).square()
    return (loss_u.mean(-1).sum() + f.square().sum() * wf) * wu


class BurgersGuidance:
    """nablaJ for GaussianDiffusion.sample(nablaJ=...): `g(x_start)` returns dJ/dx_start like get_nablaJ(loss_fn) does, from one launch and
    without a tape. `graph_safe` tells the sampler that the guided step can be captured; it is False when the kernel does not take the
    configuration (plan() raises), and the object then differentiates guidance_value like the reference.

    The two target rows J reads live in one device buffer: set_target(u_target) refills it IN PLACE, so a captured sampling step is
    replayed on the next evaluation batch's target (same batch size and width)."""

    def __init__(self, shape, ori_shape, rescaler, u_target, wu, wf, condition_f=False, wave_type='bior2.4', pad_mode='periodization',
                 is_super_model=False):
        self.shape, self.ori_shape = (int(shape[-2]), int(shape[-1])), (int(ori_shape[-2]), int(ori_shape[-1]))
        self.wu, self.wf, self.condition_f = float(wu), float(wf), bool(condition_f)
        self.wave_type, self.pad_mode, self.is_super_model = wave_type, pad_mode, bool(is_super_model)
        r = torch.as_tensor(rescaler, dtype=torch.float32).reshape(-1)
        r = r.expand(8) if r.numel() == 1 else r
        self.rescaler = r.reshape(1, -1, 1, 1)
        self._resc = {}                       # device -> the flat RESCALER there
        self._desc = {}
        self.target = None
        self.u_target = None
        self.set_target(u_target)
        try:
            plan((1, 16 if is_super_model else 8, self.shape[0], self.shape[1]), self.shape, self.ori_shape, wave_type, pad_mode, is_super_model)
            self.graph_safe = True
        except ValueError:
            self.graph_safe = False

    def key(self):
        """What a captured launch of this object bakes in besides its buffers."""
        return (self.shape, self.ori_shape, self.wu, self.wf, self.condition_f, self.wave_type, self.pad_mode, self.is_super_model)

    def set_target(self, u_target):
        n_t, n_x = self.ori_shape
        ut = torch.as_tensor(u_target)
        rows = torch.stack((ut[:, 0, :n_x], ut[:, n_t - 1, :n_x]), dim=1).to(torch.float32)
        if self.target is not None and tuple(self.target.shape) == tuple(rows.shape):
            self.target.copy_(rows)           # same storage: captured launches read the new rows
        else:
            self.target = rows.contiguous().clone()
        self.u_target = ut                    # (the autograd route reads the whole target)
        return self

    # ------------------------------------------------------------------ launches
    def _operands(self, x):
        if self.target.device != x.device:
            self.target = self.target.to(x.device)
        r = self._resc.get(x.device)
        if r is None:
            r = self._resc[x.device] = self.rescaler.reshape(-1).to(x.device).contiguous()
        if x.shape[0] != self.target.shape[0]:
            raise ValueError(f'BurgersGuidance: batch {x.shape[0]} of x against {self.target.shape[0]} target samples')
        if r.numel() < 8:
            raise ValueError(f'BurgersGuidance: RESCALER has {r.numel()} channels; the coefficient channels 0-7 are needed')
        return self.target, r

    def _launch(self, x_t, inp, t, c1, c2, s_table, clip_x0):
        from wdno_amd import _lib
        from wdno_amd.ops import _chk, _p, _stream
        inp = _chk(inp, 'x')
        key = (tuple(inp.shape), bool(clip_x0), 0 if s_table is None else int(s_table.numel()))
        d = self._desc.get(key)
        if d is None:
            pl = plan(tuple(inp.shape), self.shape, self.ori_shape, self.wave_type, self.pad_mode, self.is_super_model, self.condition_f)
            pl.pop('u_rows')
            d = _lib.BurgersGuidanceDesc(**pl, num_timesteps=key[2], condition_f=int(self.condition_f), clip_x0=int(bool(clip_x0)),
                                         wu=self.wu, wf=self.wf)
            filt = [float(v) for bank in filter_bank(self.wave_type) for v in bank]
            d = self._desc[key] = (d, (C.c_float * len(filt))(*filt))
        target, resc = self._operands(inp)
        out = torch.empty_like(inp)
        _lib.check(_lib.load().wdno_burgers_guidance(_p(x_t), _p(inp), _p(t), _p(c1), _p(c2), _p(s_table), _p(resc), _p(target), _p(out),
                                                     C.byref(d[0]), d[1], _stream()), 'wdno_burgers_guidance')
        return out

    def __call__(self, x_start):
        """dJ/dx_start (gradient mode)."""
        if not self.graph_safe:
            from ddpm_burgers.model_utils import get_nablaJ
            ut = self.u_target.to(x_start.device)
            return get_nablaJ(lambda x: guidance_value(x, ut, self.shape, self.ori_shape, self.rescaler.to(x.device), self.wu, self.wf, self.condition_f,
                                                       self.wave_type, self.pad_mode, self.is_super_model))(x_start)
        return self._launch(None, x_start.detach(), None, None, None, None, False)

    def guide(self, mod, x_t, eps, t, s_table, clip_x0):
        """One sampling step's guidance (fused mode): eps + nablaJ(x0) s_table[t] with x0 = c1[t] x_t - c2[t] eps (clamped when clip_x0),
        the schedule tables of the diffusion module `mod` and t a device int64 [B]."""
        from wdno_amd.ops import _chk
        return self._launch(_chk(x_t, 'x_t'), eps, t, mod.sqrt_recip_alphas_cumprod, mod.sqrt_recipm1_alphas_cumprod, s_table, clip_x0)


def get_nablaJ_2dconv(shape, ori_shape, RESCALER, u_target, wu=0, wf=0, condition_f=False, is_super_model=False, wave_type='bior2.4',
                      pad_mode='periodization', **unused):
    """eval_ddpm_burgers.get_nablaJ_2dconv with the reference's keyword names, minus the dataset lookup: the reference's get_target reads the
    target from the dataset files (target_i, N_upsample, dataset, device), here the caller passes u_target [B, >= n_t, >= n_x]. `args`, `low`,
    `N_upsample`, `target_i`, `device`, `dataset` are accepted and ignored (args.wave_type / args.pad_mode are read when args is given)."""
    args = unused.get('args')
    if args is not None:
        wave_type, pad_mode = getattr(args, 'wave_type', wave_type), getattr(args, 'pad_mode', pad_mode)
    return BurgersGuidance(shape, ori_shape, RESCALER, u_target, wu, wf, condition_f=condition_f, wave_type=wave_type, pad_mode=pad_mode,
                           is_super_model=is_super_model)
