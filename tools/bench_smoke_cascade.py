"""Timings of the smoke super-resolution cascade's pieces on one GPU (profiles/smoke_cascade.md), each against the torch chain of the
reference's lines on this tree's operators, at the reference's size: base sample [B, 24, 42, 40, 40] with block (18, 34, 34), super sample
[B, 24, 82, 80, 80] with block (18, 66, 66), fields (32, 128, 128).

  --conditions    wdno_amd.smoke.cascade.super_conditions (two launches) against run_super_model l.172-196 plus the three copies of
                  GaussianDiffusion._condition_source
  --reconstruct   the level-1 reconstruct (offset 1, rows split at 40) against the chain of l.213-231
  --score         wdno_amd.smoke.score.score_super against multi_evaluate's super branch l.405-456 on torch, with the peak device memory of each
  --cascade       one whole cascade batch (InferencePipeline.run_model) with random-weight full-size models and `--steps` DDIM steps per level:
                  wall time, and the share spent in the two sample() calls
Device events around `--iters` back-to-back calls per window, 5 windows, the arms alternating inside each window, every arm run once
untimed, one process; spread = (max - min) / median. Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import tempfile
import time
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wdno_amd import tree_path  # noqa: E402

for _t in ('third_party', 'smoke'):
    sys.path.insert(0, tree_path(_t))
from ddpm.wave_utils import upsample_coef  # noqa: E402
from wave_trans_2d import coef_to_tensor, tensor_to_coef  # noqa: E402
from wdno_amd import wavelets as W  # noqa: E402
from wdno_amd.smoke.cascade import super_conditions  # noqa: E402
from wdno_amd.smoke.reconstruct import reconstruct  # noqa: E402
from wdno_amd.smoke.score import score_super  # noqa: E402

SHAPE, ORI = [(18, 34, 34), (18, 66, 66)], [(32, 64, 64), (32, 128, 128)]
PAD_T, PAD_X = 24, 80


def _resc():
    return torch.linspace(1.0, 9.0, 82, device='cuda').reshape(1, 1, 82, 1, 1)


def chain_conditions(prev, fine, resc):
    """l.172-196 and the assembly of the sampler's condition source (diffusion_2d.py: _condition_source)."""
    coef = tensor_to_coef(prev[:, :, :40].permute(0, 2, 1, 3, 4), SHAPE[0])
    ret = coef_to_tensor(coef).reshape(-1, 5, 8, *SHAPE[0]).reshape(-1, 40, *SHAPE[0]).permute(0, 2, 1, 3, 4)
    nx = SHAPE[1][-2]
    yl0, yh0 = W.DWTForward(J=1, mode='zero', wave='bior1.3')(fine[:, 0, [0]].contiguous())
    wave_init = torch.cat((yl0, yh0[0][:, 0]), dim=1)
    wave_init = wave_init.unsqueeze(1).expand(wave_init.shape[0], PAD_T // 4, 4, nx, nx).reshape(-1, PAD_T, nx, nx)
    wave_init = F.pad(wave_init, (0, PAD_X - nx, 0, PAD_X - nx), 'constant', 0)
    wc = W.wavedec3(fine[:, :, 3:5].permute(0, 2, 1, 3, 4).reshape(-1, fine.shape[1], fine.shape[3], fine.shape[4]).contiguous(), 'bior1.3', mode='zero', level=1)
    wc = coef_to_tensor(wc)
    wc = F.pad(wc.reshape(-1, *wc.shape[-3:]), (1, 1, 1, 1), mode='replicate')
    wc = F.pad(wc, (0, PAD_X - wc.shape[-1], 0, PAD_X - wc.shape[-2], 0, PAD_T - wc.shape[-3]), 'constant', 0) \
        .reshape(-1, 2, 8, PAD_T, PAD_X, PAD_X).reshape(-1, 16, PAD_T, PAD_X, PAD_X).permute(0, 2, 1, 3, 4)
    low = upsample_coef(ret.contiguous(), SHAPE[1], type='space')
    low = F.pad(low, (0, PAD_X - low.shape[-1], 0, PAD_X - low.shape[-2], 0, 0, 0, PAD_T - low.shape[-4]), 'constant', 0)
    src = torch.zeros(prev.shape[0], PAD_T, 82, PAD_X, PAD_X, device=prev.device)
    src[:, :, -2] = wave_init / resc[:, :, -2]
    src[:, :, 24:40] = wc / resc[:, :, 24:40]
    src[:, :, 40:80] = low
    return src


def chain_reconstruct(x, resc):
    """l.213-231 for level 1."""
    shape, ori = SHAPE[1], ORI[1]
    wave_output = x[:, :, :40] * resc[:, :, :40]
    coef = tensor_to_coef(wave_output.permute(0, 2, 1, 3, 4), shape, upsample_type='space')
    rec = W.waverec3([coef[0].contiguous(), {k: v.contiguous() for k, v in coef[1].items()}], 'bior1.3', 'zero')
    ori_output = rec[:, :ori[0], :ori[1], :ori[2]].reshape(-1, 5, *ori).permute(0, 2, 1, 3, 4)
    so = x[:, :, [-1]] * resc[:, :, [-1]]
    half = int(wave_output.shape[-2] / 2)
    lo = so[:, :shape[0], -1, :half].mean((-2, -1)).unsqueeze(1)
    hi = so[:, :shape[0], -1, half:].mean((-2, -1)).unsqueeze(1)
    smoke_out = W.DWT1DInverse(mode='zero', wave='bior1.3')((lo.contiguous(), [hi.contiguous()]))[:, 0]
    smoke_out = smoke_out[:, :ori[0]].reshape(smoke_out.shape[0], ori[0], 1, 1, 1).expand(-1, -1, -1, ori[1], ori[2])
    return torch.cat((ori_output, smoke_out), dim=2)


def chain_score(pred, data, w_energy):
    """multi_evaluate's super branch in simulation mode, l.405-456, on torch (the four-entry arrays)."""
    pred = pred.clone()
    data_current = data[:, :, :, ::int(data.shape[-1] / pred.shape[-1]), ::int(data.shape[-1] / pred.shape[-1])]
    data_base = data[:, :, :, ::2, ::2]
    pred_base = pred[:, :, :, ::int(pred.shape[-1] / 64), ::int(pred.shape[-1] / 64)]
    flat = pred.reshape(pred.shape[0], -1, *pred.shape[-2:])
    pred_super = F.interpolate(flat, size=(128, 128), mode='bilinear', align_corners=False).reshape(pred.shape[0], pred.shape[1], pred.shape[2], 128, 128)
    pred_super2 = F.interpolate(flat, size=(128, 128), mode='nearest').reshape(pred.shape[0], pred.shape[1], pred.shape[2], 128, 128)
    out = []
    for p, d in ((pred_base, data_base), (pred, data_current), (pred_super, data), (pred_super2, data)):
        mask = torch.ones_like(p)
        mask[:, 0, 0] = False
        p, d = p * mask, d * mask
        e = p - d
        mse_wo = e[:, :, :3].square().mean((1, 2, 3, 4)).cpu().numpy()
        n_l2 = (e[:, :, :3].square().sum((1, 2, 3, 4)).sqrt() / d[:, :, :3].square().sum((1, 2, 3, 4)).sqrt()).cpu().numpy()
        j_t = -d[:, -1, -1, 0, 0].cpu().numpy()
        j_e = d[:, :, 3:5].square().mean((1, 2, 3, 4)).cpu().numpy()
        out.append((float((j_t + w_energy * j_e).mean()), float(j_t.mean()), float(j_e.mean()), float(mse_wo.mean()), float(n_l2.mean())))
    return np.array(out).T


def _window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _arms(what, batch, iters, arms, rel):
    t = {k: [] for k in arms}
    for _ in range(5):
        for k, fn in arms.items():
            t[k].append(_window(fn, iters))
    out = dict(what=what, batch=batch, iters=iters, kernel_vs_chain_relmax=rel)
    for k, v in t.items():
        med = float(np.median(v))
        out[k] = dict(median_ms=med, spread_pct=100 * (max(v) - min(v)) / med, windows_ms=[round(w, 4) for w in v])
    out['ratio_chain_over_kernel'] = out['chain']['median_ms'] / out['kernel']['median_ms']
    print(json.dumps(out), flush=True)


def _gen(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


def bench_conditions(batch, iters):
    prev = torch.randn(batch, 24, 42, 40, 40, device='cuda', generator=_gen(1)) * 0.4
    fine = torch.randn(batch, 32, 6, 128, 128, device='cuda', generator=_gen(2))
    resc = _resc()
    arms = {'kernel': lambda: super_conditions(prev, SHAPE[0], fine, resc, SHAPE[1], PAD_T, PAD_X), 'chain': lambda: chain_conditions(prev, fine, resc)}
    a, b = arms['kernel'](), arms['chain']()
    _arms('conditions', batch, iters, arms, float((a - b).abs().max() / b.abs().max()))


def bench_reconstruct(batch, iters):
    x = torch.randn(batch, 24, 82, 80, 80, device='cuda', generator=_gen(3)) * 0.4
    resc = _resc()
    arms = {'kernel': lambda: reconstruct(x, SHAPE[1], ORI[1], resc, upsample_type='space', half=40), 'chain': lambda: chain_reconstruct(x, resc)}
    a, b = arms['kernel'](), arms['chain']()
    _arms('reconstruct_level1', batch, iters, arms, float((a - b).abs().max() / b.abs().max()))


def bench_score(batch, iters, w_energy=0.7):
    data = torch.randn(batch, 32, 6, 128, 128, device='cuda', generator=_gen(4))
    for n in (64, 128):
        pred = torch.randn(batch, 32, 6, n, n, device='cuda', generator=_gen(5))
        arms = {'kernel': lambda: score_super(pred, data, w_energy), 'chain': lambda: chain_score(pred, data, w_energy)}
        peak = {}
        for k, fn in arms.items():
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            r = fn()
            torch.cuda.synchronize()
            peak[k] = (torch.cuda.max_memory_allocated() - base, r)
        ra = np.stack([peak['kernel'][1][k].mean(1) for k in ('J_total', 'J_target', 'J_energy', 'mse_wo_smoke', 'n_l2')])
        rel = float(np.abs(ra - peak['chain'][1]).max() / np.abs(peak['chain'][1]).max())
        print(json.dumps(dict(what=f'score_peak_bytes_above_inputs_pred{n}', batch=batch, kernel=peak['kernel'][0], chain=peak['chain'][0])), flush=True)
        _arms(f'score_super_pred{n}', batch, iters, arms, rel)


def bench_cascade(batch, steps):
    import inference_2d as INF
    from ddpm.diffusion_2d import GaussianDiffusion
    from video_diffusion_pytorch.video_diffusion_pytorch_conv3d import Unet3D_with_Conv3D
    from wdno_amd.smoke.guidance import CascadeGuidance, SmokeGuidance
    torch.manual_seed(0)
    resc = _resc()
    kw = dict(loss_layer_weight=None, is_condition_control=True, is_condition_pad=True, is_wavelet=True, wave_type='bior1.3', pad_mode='zero',
              image_size=40, frames=24, timesteps=1000, sampling_timesteps=steps, ddim_sampling_eta=1.0, standard_fixed_ratio=0.05, coeff_ratio=0.3)
    shape, ori = [list(s) for s in SHAPE], [list(o) for o in ORI]
    m0 = GaussianDiffusion(Unet3D_with_Conv3D(dim=64, dim_mults=(1, 2, 4), channels=42), is_super_model=False, padded_shape=shape[0], ori_shape=ori[0], **kw).cuda()
    m1 = GaussianDiffusion(Unet3D_with_Conv3D(dim=64, dim_mults=(1, 2, 4), channels=82), is_super_model=True, padded_shape=shape, ori_shape=ori, **kw).cuda()
    gk = dict(is_condition_control=True, w_energy=0.7, w_init=0.4)
    fn = CascadeGuidance([SmokeGuidance(shape[0], ori[0], resc[:, :, 40:], **gk), SmokeGuidance(shape[1], ori[1], resc, **gk)])
    args = types.SimpleNamespace(is_wavelet=True, is_condition_control=True, image_size=64, device='cuda', upsample=1, is_super_model=True, w_energy=0.7)
    ppl = INF.InferencePipeline([m0, m1], {'design_fn': fn, 'design_guidance': 'standard'}, resc, results_path=tempfile.mkdtemp(prefix='wdno_bench_cascade_'), args_general=args)
    state = torch.randn(batch, 32, 6, 128, 128, generator=torch.Generator().manual_seed(6))
    spent = [0.0]
    for m in (m0, m1):
        def timed(inner=m.sample, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = inner(**k)
            torch.cuda.synchronize()
            spent[0] += time.perf_counter() - t0
            return out
        m.sample = timed
    rows = []
    for _ in range(3):                                   # the first pass captures the step graphs
        spent[0] = 0.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        preds = ppl.run_model(state)
        for p in preds:
            ppl.multi_evaluate(p, state)
        torch.cuda.synchronize()
        rows.append((time.perf_counter() - t0, spent[0]))
    print(json.dumps(dict(what='cascade_batch', batch=batch, ddim_steps=steps, passes_s=[round(r[0], 4) for r in rows], sampling_s=[round(r[1], 4) for r in rows],
                          sampling_share_last=rows[-1][1] / rows[-1][0])), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    for flag in ('--conditions', '--reconstruct', '--score', '--cascade'):
        ap.add_argument(flag, action='store_true')
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--steps', type=int, default=4)
    a = ap.parse_args()
    if a.conditions:
        bench_conditions(a.batch, a.iters)
    if a.reconstruct:
        bench_reconstruct(a.batch, a.iters)
    if a.score:
        bench_score(a.batch, a.iters)
    if a.cascade:
        bench_cascade(a.batch, a.steps)
