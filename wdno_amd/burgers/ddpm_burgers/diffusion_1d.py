"""GaussianDiffusion (Burgers, 2-D (t, x) wavelet-coefficient images) on MI355X -- drop-in for
burgers/ddpm_burgers/diffusion_1d.py:40-654.

Same constructor signature (train_ddpm_burgers.py:158-181), attributes, buffer names and methods as the reference.
Execution differs: q_sample + every set_condition overwrite + the masked target are ONE launch in training
(diffusion_1d.py:542-637 is ~25 indexed assignments); a sampling step is the U-Net plus two launches (update, re-impose
conditions). The noise source is `self.sample_noise` so tests can replay the reference's draws.

Scope: the wavelet parametrisation with objective='pred_noise' (the only configuration the WDNO scripts use).
"""
import math
from collections import namedtuple

import torch
from torch import nn

from wdno_amd import diffusion_core as K
from ddpm_burgers.model_utils import default, extract, identity, normalize_to_neg_one_to_one, unnormalize_to_zero_to_one
from ddpm_burgers.model_utils import cosine_beta_schedule, linear_beta_schedule

ModelPrediction = namedtuple('ModelPrediction', ['pred_noise', 'pred_x_start'])


class GaussianDiffusion(nn.Module):
    def __init__(
        self,
        model,
        *,
        seq_length,
        is_wavelet=True,
        pad_mode=None,
        wave_type=None,
        padded_shape=None,
        ori_shape=torch.tensor([81, 128]),      # the reference default (diffusion_1d.py:51, there on 'cuda')
        is_super_model=False,
        upsample_t=1,
        upsample_x=1,
        timesteps=1000,
        sampling_timesteps=None,
        objective='pred_noise',
        beta_schedule='cosine',
        ddim_sampling_eta=0.,
        auto_normalize=False,
        loss_layer_weight=1,
        is_condition_pad=True,
        is_condition_u0=False,
        is_condition_uT=False,
        is_condition_f=False,
        train_on_padded_locations=True,
    ):
        super().__init__()
        if not is_wavelet:
            raise NotImplementedError('wdno_amd implements the wavelet parametrisation only (is_wavelet=True)')
        assert objective in {'pred_noise', 'pred_x0', 'pred_v'}, 'objective must be either pred_noise (predict noise) or pred_x0 (predict image start) or pred_v (predict v)'
        self.is_wavelet = is_wavelet
        self.is_super_model = is_super_model
        self.pad_mode = pad_mode
        self.wave_type = wave_type
        self.model = model
        self.channels = self.model.channels
        self.self_condition = self.model.self_condition
        self.traj_size = seq_length
        self.objective = objective

        if beta_schedule == 'linear':
            betas = linear_beta_schedule(timesteps)
        elif beta_schedule == 'cosine':
            betas = cosine_beta_schedule(timesteps)
        else:
            raise ValueError(f'unknown beta schedule {beta_schedule}')
        timesteps, = betas.shape
        self.num_timesteps = int(timesteps)
        self.sampling_timesteps = default(sampling_timesteps, timesteps)
        assert self.sampling_timesteps <= timesteps
        self.is_ddim_sampling = self.sampling_timesteps < timesteps
        self.ddim_sampling_eta = ddim_sampling_eta

        # loss weight per objective (diffusion_1d.py:147-156). pred_noise is the WDNO path (fused launches); pred_x0 / pred_v keep the
        # reference's semantics on the same U-Net kernels with torch element-wise glue around them (round 3).
        lw = {'pred_noise': lambda snr: torch.ones_like(snr), 'pred_x0': lambda snr: snr, 'pred_v': lambda snr: snr / (snr + 1)}[objective]
        alphas, _ = K.register_schedule(self, betas, lw)
        self.alphas = alphas.to(torch.float32).clone()
        self.alphas_prev = torch.nn.functional.pad(alphas[:-1], (1, 0), value=1.).to(torch.float32).clone()

        self.normalize = normalize_to_neg_one_to_one if auto_normalize else identity
        self.unnormalize = unnormalize_to_zero_to_one if auto_normalize else identity
        self.loss_layer_weight = loss_layer_weight
        self.upsample_t = upsample_t
        self.upsample_x = upsample_x
        self.is_condition_pad = is_condition_pad
        self.is_condition_u0 = is_condition_u0
        self.is_condition_uT = is_condition_uT
        self.is_condition_f = is_condition_f
        self.train_on_padded_locations = train_on_padded_locations
        self.padded_shape = padded_shape
        self.ori_shape = ori_shape
        self._wc_cache = None
        self.use_graph = None       # None: HIP-graph replay of the unguided sampling step when the loop is long enough (WDNO_SAMPLE_GRAPH)

    # ------------------------------------------------------------------ helpers
    @property
    def _ac_host(self):
        return K.ac_host(self)          # host copy of the current alphas_cumprod buffer (scalar DDIM coefficients)

    def sample_noise(self, shape, device):
        return torch.randn(tuple(shape), device=device)

    def _desc(self, shape, coef_shape, u_rows, uT_rows):
        return K.cond_desc(1, tuple(shape), [int(coef_shape[0]), int(coef_shape[1])], self.is_condition_pad, self.is_condition_u0,
                           self.is_condition_uT, self.is_condition_f, self.is_super_model, u_rows, uT_rows)

    def _channel_weights(self, c, device):
        lw = self.loss_layer_weight
        key = (id(lw), c, str(device))
        if self._wc_cache is None or self._wc_cache[0] != key:
            w = torch.as_tensor(lw, dtype=torch.float32).reshape(-1)
            w = w.expand(c) if w.numel() == 1 else w
            assert w.numel() == c, 'loss_layer_weight must be a scalar or [1, C, 1, 1]'
            self._wc_cache = (key, w.to(device).contiguous())
        return self._wc_cache[1]

    # ------------------------------------------------------------------ closed-form pieces (API parity)
    def predict_start_from_noise(self, x_t, t, noise):
        return extract(self.sqrt_recip_alphas_cumprod, t, x_t.shape) * x_t - extract(self.sqrt_recipm1_alphas_cumprod, t, x_t.shape) * noise

    def predict_noise_from_start(self, x_t, t, x0):
        return (extract(self.sqrt_recip_alphas_cumprod, t, x_t.shape) * x_t - x0) / extract(self.sqrt_recipm1_alphas_cumprod, t, x_t.shape)

    def predict_v(self, x_start, t, noise):
        return extract(self.sqrt_alphas_cumprod, t, x_start.shape) * noise - extract(self.sqrt_one_minus_alphas_cumprod, t, x_start.shape) * x_start

    def predict_start_from_v(self, x_t, t, v):
        return extract(self.sqrt_alphas_cumprod, t, x_t.shape) * x_t - extract(self.sqrt_one_minus_alphas_cumprod, t, x_t.shape) * v

    def q_posterior(self, x_start, x_t, t):
        mean = extract(self.posterior_mean_coef1, t, x_t.shape) * x_start + extract(self.posterior_mean_coef2, t, x_t.shape) * x_t
        return mean, extract(self.posterior_variance, t, x_t.shape), extract(self.posterior_log_variance_clipped, t, x_t.shape)

    @torch.no_grad()
    def interpolate(self, x1, x2, t=None, lam=0.5):
        """diffusion_1d.py:500-518: noise both ends to step t, blend, denoise back with p_sample (no conditioning, as in the reference)."""
        b, device = x1.shape[0], x1.device
        t = default(t, self.num_timesteps - 1)
        assert x1.shape == x2.shape
        t_batched = torch.full((b,), t, device=device, dtype=torch.long)
        xt1, xt2 = (self.q_sample(v, t=t_batched) for v in (x1, x2))
        img = (1 - lam) * xt1 + lam * xt2
        x_start = None
        for i in reversed(range(0, t)):
            self_cond = x_start if self.self_condition else None
            img, x_start, _ = self.p_sample(img.contiguous(), i, self_cond)
        return img

    def get_guidance_options(self, **kwargs):
        nabla_J = kwargs.get('nablaJ')
        if nabla_J is not None:
            assert not self.self_condition, 'self condition not tested with guidance'
        sched = kwargs.get('J_scheduler') or (lambda t: 1.)
        proj = kwargs.get('proj_guidance') or (lambda ep, nj: ep + nj)
        return nabla_J, sched, proj

    def set_condition(self, img, u, shape, condition_type):
        """In-place overwrite with the reference's indexing (diffusion_1d.py:276-288). Kept for API parity; the training
        and sampling loops below use the fused predicate kernel instead."""
        if condition_type == 'u0':
            img[:, -1, :u.shape[-2], :shape[-1]] = u[:, :, :shape[-1]]
        elif condition_type == 'uT':
            img[:, -1, -u.shape[-2]:, :shape[-1]] = u[:, :, :shape[-1]]
        elif condition_type == 'f':
            img[:, 4:8, :shape[-2], :shape[-1]] = u[:, :, :shape[-2], :shape[-1]]
        elif condition_type == 'low':
            img[:, 8:16, :shape[-2], :shape[-1]] = u[:, :, :shape[-2], :shape[-1]]
        elif condition_type == 'pad':
            img[:, :-1, shape[-2]:] = 0
            img[:, :, :, shape[-1]:] = 0
        else:
            raise ValueError(condition_type)

    # ------------------------------------------------------------------ sampling
    def model_predictions(self, x, t, x_self_cond=None, clip_x_start=False, rederive_pred_noise=False, **kwargs):
        model_output = self.model(x, t, x_self_cond)
        maybe_clip = (lambda v: v.clamp(-1., 1.)) if clip_x_start else identity
        nabla_J, sched, proj = self.get_guidance_options(**kwargs)
        if self.objective == 'pred_x0':            # diffusion_1d.py:229-232
            x_start = maybe_clip(model_output)
            return ModelPrediction(self.predict_noise_from_start(x, t, x_start), x_start)
        if self.objective == 'pred_v':             # :234-238
            x_start = maybe_clip(self.predict_start_from_v(x, t, model_output))
            return ModelPrediction(self.predict_noise_from_start(x, t, x_start), x_start)
        pred_noise = kwargs['pred_noise'] if kwargs.get('pred_noise') is not None else model_output
        x_start = maybe_clip(self.predict_start_from_noise(x, t, pred_noise))
        if nabla_J is not None:
            with torch.enable_grad():
                pred_noise = proj(pred_noise, nabla_J(x_start) * sched(t[0].item()))
            x_start = maybe_clip(self.predict_start_from_noise(x, t, pred_noise))
        if clip_x_start and rederive_pred_noise:
            pred_noise = self.predict_noise_from_start(x, t, x_start)
        return ModelPrediction(pred_noise, x_start)

    def p_mean_variance(self, x, t, x_self_cond=None, **kwargs):
        preds = self.model_predictions(x, t, x_self_cond, **kwargs)
        x_start = preds.pred_x_start.clamp(-1., 1.)
        mean, var, logvar = self.q_posterior(x_start=x_start, x_t=x, t=t)
        return mean, var, logvar, x_start, preds.pred_noise

    def _guided(self, kwargs):
        """Does the step need the general (torch element-wise) form? Guidance, an injected pred_noise, or an objective other than pred_noise:
        the fused posterior / DDIM update launches take the U-Net output as the noise estimate."""
        return self.objective != 'pred_noise' or any(kwargs.get(k) is not None for k in ('nablaJ', 'pred_noise'))

    def _graph_guidance(self, kwargs):
        """Guidance the fused, graph-replayed loop takes (K.guided_sampling_loop_burgers): a `graph_safe` objective with a fused step
        (burgers/guidance.py: BurgersGuidance), the default projection eps + nablaJ s, the U-Net's own noise estimate. Everything else --
        plain callables, a custom proj_guidance, an injected pred_noise, pred_x0 / pred_v, self-conditioning -- keeps the general form."""
        nabla_J = kwargs.get('nablaJ')
        return (self.objective == 'pred_noise' and nabla_J is not None and bool(getattr(nabla_J, 'graph_safe', False))
                and hasattr(nabla_J, 'guide') and kwargs.get('proj_guidance') is None and kwargs.get('pred_noise') is None
                and not self.self_condition)

    def _guided_loop(self, img, src, desc, kwargs, **loop):
        s_table = K.guidance_s_table(kwargs.get('J_scheduler'), self.num_timesteps)
        return K.guided_sampling_loop_burgers(self, img, src, desc, kwargs['nablaJ'], s_table, use_graph=self.use_graph, **loop)

    @torch.no_grad()
    def p_sample(self, x, t: int, x_self_cond=None, **kwargs):
        b, device = x.shape[0], x.device
        bt = torch.full((b,), t, device=device, dtype=torch.long)
        noise = self.sample_noise(x.shape, device) if t > 0 else None
        if not self._guided(kwargs):
            eps = self.model(x, bt, x_self_cond)
            x_next, x_start = K.p_sample_update(self, x, eps, noise, bt, clamp=True)
            return x_next, x_start, eps
        mean, _, logvar, x_start, pred_noise = self.p_mean_variance(x=x, t=bt, x_self_cond=x_self_cond, **kwargs)
        pred = mean if noise is None else mean + (0.5 * logvar).exp() * noise
        return pred, x_start, pred_noise

    _cond_src = None

    def sample_with_source(self, cond_src, **kwargs):
        """sample(**kwargs) with the condition source handed over assembled (an extension; sample, p_sample_loop and ddim_sample keep the
        reference's parameter lists): cond_src is a contiguous fp32 tensor of the sampled shape on the sampling device whose conditioned
        positions hold the clean values (burgers/cascade.py: super_conditions). It is used as it is instead of a zeroed tensor and the
        copies; low, u_init and u_final are still passed, as views of it, for the shapes."""
        self._cond_src = cond_src
        try:
            return self.sample(**kwargs)
        finally:
            self._cond_src = None

    def _sampling_setup(self, shape, kwargs):
        device = self.betas.device
        if not self.is_super_model:
            coef_shape = self.padded_shape
        else:
            ps = self.padded_shape[kwargs['N_upsample'] - 1]
            coef_shape = [ps[0] + 1, ps[1]]
        cw = int(coef_shape[-1])
        cond_src = self._cond_src
        if cond_src is not None:                # handed over assembled (sample_with_source): the conditions give the shapes only
            if tuple(cond_src.shape) != tuple(shape) or cond_src.dtype != torch.float32 or cond_src.device != torch.device(device) or \
                    not cond_src.is_contiguous():
                raise ValueError(f'cond_src must be a contiguous float32 {tuple(shape)} tensor on {device}, got {cond_src.dtype} '
                                 f'{tuple(cond_src.shape)} on {cond_src.device}')
            u_rows = kwargs['u_init'].shape[-2] if self.is_condition_u0 else 0
            uT_rows = kwargs['u_final'].shape[-2] if self.is_condition_uT else 0
            return cond_src, self._desc(shape, coef_shape, u_rows, uT_rows)
        src = torch.zeros(tuple(shape), device=device, dtype=torch.float32)
        u_rows = uT_rows = 0
        if self.is_condition_u0:
            u0 = kwargs['u_init'].to(device)
            u_rows = u0.shape[-2]
            src[:, -1, :u_rows, :cw] = u0[:, :, :cw]
        if self.is_condition_uT:
            uT = kwargs['u_final'].to(device)
            uT_rows = uT.shape[-2]
            src[:, -1, -uT_rows:, :cw] = uT[:, :, :cw]
        ch = int(coef_shape[-2])
        if self.is_condition_f:
            f = kwargs['f'].to(device)
            src[:, 4:8, :ch, :cw] = f[:, :, :ch, :cw]
        if self.is_super_model:
            low = kwargs['low'].to(device)
            src[:, 8:16, :ch, :cw] = low[:, :, :ch, :cw]
        return src, self._desc(shape, coef_shape, u_rows, uT_rows)

    @torch.no_grad()
    def p_sample_loop(self, shape, **kwargs):
        device = self.betas.device
        src, desc = self._sampling_setup(shape, kwargs)
        img = self.sample_noise(shape, device).contiguous()
        if not self._guided(kwargs) and not self.self_condition:   # unguided: fused launches, the step replayed from one HIP graph
            img = K.sampling_loop(self, img, src, desc, cond_first=True, use_graph=self.use_graph)
        elif self._graph_guidance(kwargs):                         # the control objective's kernel: the same, one launch more per step
            img = self._guided_loop(img, src, desc, kwargs)
        else:
            x_start = None
            for t in reversed(range(0, self.num_timesteps)):
                K.apply_cond(img, src, desc)
                self_cond = x_start if self.self_condition else None
                img, x_start, _ = self.p_sample(img, t, self_cond, **kwargs)
                img = img.detach().contiguous()
        K.apply_cond(img, src, desc)
        return self.unnormalize(img)

    @torch.no_grad()
    def ddim_sample(self, shape, **kwargs):
        device, eta = self.betas.device, self.ddim_sampling_eta
        batch = shape[0]
        src, desc = self._sampling_setup(shape, kwargs)
        img = self.sample_noise(shape, device).contiguous()
        pairs = K.ddim_time_pairs(self.num_timesteps, self.sampling_timesteps)
        if not self._guided(kwargs) and not self.self_condition:
            img = K.sampling_loop(self, img, src, desc, ddim_pairs=pairs, eta=eta, cond_first=True, use_graph=self.use_graph)
        elif self._graph_guidance(kwargs):
            img = self._guided_loop(img, src, desc, kwargs, ddim_pairs=pairs, eta=eta)
        else:
            x_start = None
            for time, time_next in pairs:
                K.apply_cond(img, src, desc)
                tc = torch.full((batch,), time, device=device, dtype=torch.long)
                self_cond = x_start if self.self_condition else None
                pred_noise, x_start, *_ = self.model_predictions(img, tc, self_cond, clip_x_start=True, rederive_pred_noise=True, **kwargs)
                if time_next < 0:
                    img = x_start.contiguous()
                    continue
                sigma, c, sqrt_an = K.ddim_coefficients(self._ac_host, time, time_next, eta)
                img = (x_start * sqrt_an + c * pred_noise + sigma * self.sample_noise(shape, device)).contiguous()
        K.apply_cond(img, src, desc)
        return self.unnormalize(img)

    def sample(self, batch_size=16, **kwargs):
        if self.is_condition_u0:
            assert 'is_condition_u0' not in kwargs, 'specify this value in the model. not during sampling.'
            assert kwargs.get('u_init') is not None
        if self.is_condition_uT:
            assert 'is_condition_uT' not in kwargs, 'specify this value in the model. not during sampling.'
            assert kwargs.get('u_final') is not None
        if self.is_condition_f:
            assert 'is_condition_f' not in kwargs, 'specify this value in the model. not during sampling.'
            assert kwargs.get('f') is not None
        if self.is_super_model:
            assert kwargs.get('N_upsample') is not None and kwargs.get('low') is not None
        if not self.is_super_model:
            sample_size = (batch_size, self.channels, *self.traj_size)
        else:
            sample_size = (batch_size, self.channels, *kwargs['low'].shape[-2:])
        fn = self.p_sample_loop if not self.is_ddim_sampling else self.ddim_sample
        return fn(sample_size, **kwargs)

    # ------------------------------------------------------------------ training
    def q_sample(self, x_start, t, noise=None):
        noise = default(noise, lambda: torch.randn_like(x_start))
        x, _ = K.q_sample_cond(x_start, noise, t, self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod, K.plain_desc(x_start))
        return x

    def p_losses(self, x_start, t, noise=None):
        b, c, nt, nx = x_start.shape
        if self.is_super_model:
            n_down = int(math.log2(64 / nx))
            coef_shape = [self.padded_shape[n_down][0] + 1, self.padded_shape[n_down][1]]
        else:
            coef_shape = self.padded_shape
        noise = default(noise, lambda: self.sample_noise(x_start.shape, x_start.device))
        if self.self_condition:
            raise NotImplementedError('self-conditioning is never enabled on the WDNO path')
        desc = self._desc(x_start.shape, coef_shape, int(nt / 2), nt - int(nt / 2))
        x, target = K.q_sample_cond(x_start, noise, t, self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod, desc)
        model_out = self.model(x, t, None)
        if self.objective == 'pred_x0':            # diffusion_1d.py:596-602: the target is taken BEFORE the conditioned regions of `noise` are zeroed,
            target = x_start                       # so only the pred_noise target carries the mask
        elif self.objective == 'pred_v':
            target = self.predict_v(x_start, t, noise)
        wc = self._channel_weights(c, x.device)
        wb = self.loss_weight[t].contiguous()
        # mean_b( mean_{c,h,w}((out - target)^2 * w[c]) * loss_weight[t_b] )
        return K.weighted_mse(model_out, target, wc, wb, c, nt * nx)

    def forward(self, img, *args, **kwargs):
        b, device = img.shape[0], img.device
        t = torch.randint(0, self.num_timesteps, (b,), device=device).long()
        img = self.normalize(img)
        return self.p_losses(img, t, *args, **kwargs)


class GaussianDiffusion1D(GaussianDiffusion):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
