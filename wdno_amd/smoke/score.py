"""The metrics of the smoke inference on the GPU: InferencePipeline.multi_evaluate's arithmetic (smoke/inference_2d.py:426-439) as one launch
of csrc/smoke_score.hip (include/wdno_hip.h: wdno_smoke_score) that reads only the frames and cells the metrics read.

The reference scores a control by building solver_out [B, 256, 6, 128, 128] in fp64 on the host (10 GB at the inference batch of 50),
uploading it and keeping one frame in 8 and one cell in 4. Here the data is described per channel -- a base pointer, the element strides of
sample / frame / row / column and the element type; a zero stride broadcasts -- so the six channels may live in different arrays and
nothing is gathered: the solver writes only the T frames (smoke_solver.solve(frames=...)), its density and velocity are read at stride 2,
the masked controls of pred itself serve as channels 3 and 4 (tiling by (8, 2) and taking ::8, ::2, ::2 is the identity) and the fp64
ratio [B, 256] is read at frame stride 256 // T with zero spatial strides.

score()          -- the launch and the metric formulas on its five fp64 sums per sample.
score_controls() -- control mode: the indirect-control copy of pred, the frames-only solve, score().
score_super()    -- simulation mode of a cascade level (smoke/inference_2d.py:405-456): the four comparisons base / current / linear / nearest
                    from one launch (wdno_smoke_score_super). The reference interpolates pred to two [B, T, 6, 128, 128] tensors, masks eight
                    tensors and reduces each four times; here the kernel samples pred through the interpolation while it reads the data in place.
"""
import ctypes as C

import numpy as np
import torch

KEYS = ('mse', 'mse_wo_smoke', 'n_l2', 'J_target', 'J_energy', 'J_total')


def _channel_table(data_channels, shape, device):
    from wdno_amd import _lib
    B, T, h, w = shape
    if len(data_channels) != 6:
        raise ValueError(f'smoke score: six data channels expected, got {len(data_channels)}')
    table = (_lib.SmokeScoreChannel * 6)()
    for c, d in enumerate(data_channels):
        if not torch.is_tensor(d) or d.device != device or d.dtype not in (torch.float32, torch.float64):
            raise ValueError(f'smoke score: data channel {c} must be a float32 or float64 tensor on {device}')
        if tuple(d.shape) != (B, T, h, w):
            raise ValueError(f'smoke score: data channel {c} is {tuple(d.shape)}, pred needs a (broadcast) view of {(B, T, h, w)}')
        st = [0 if n == 1 else int(s) for n, s in zip(d.shape, d.stride())]
        if min(st) < 0:
            raise ValueError(f'smoke score: data channel {c} has a negative stride')
        table[c] = _lib.SmokeScoreChannel(d.data_ptr(), st[0], st[1], st[2], st[3], int(d.dtype == torch.float64), 0)
    return table


def score(pred, data_channels, w_energy):
    """pred [B, T, 6, h, w] fp32 on the GPU; data_channels: six tensors on pred's device, each a view (strided, expanded) of shape
    [B, T, h, w], fp32 or fp64. Returns {key: fp64 numpy [B]} for KEYS, the per-sample values whose batch means multi_evaluate reports."""
    from wdno_amd import _lib
    from wdno_amd.ops import _p, _stream
    if not pred.is_cuda or pred.dtype != torch.float32 or pred.dim() != 5 or pred.shape[2] != 6:
        raise RuntimeError(f'smoke score: pred must be a float32 [B, T, 6, h, w] tensor on the GPU, got {pred.dtype} {tuple(pred.shape)} on {pred.device}')
    pred = pred.detach().contiguous()
    B, T, _, h, w = (int(v) for v in pred.shape)
    table = _channel_table(data_channels, (B, T, h, w), pred.device)
    with torch.cuda.device(pred.device):
        out = torch.empty(B, 5, dtype=torch.float64, device=pred.device)
        _lib.check(_lib.load().wdno_smoke_score(_p(pred), table, _p(out), B, T, h, w, _stream()), 'wdno_smoke_score')
    s = out.cpu().numpy()
    cells = T * h * w
    j_target, j_energy = -s[:, 4], s[:, 3] / (2 * cells)
    return dict(mse=(s[:, 0] + s[:, 1]) / (4 * cells), mse_wo_smoke=s[:, 0] / (3 * cells), n_l2=np.sqrt(s[:, 0]) / np.sqrt(s[:, 2]),
                J_target=j_target, J_energy=j_energy, J_total=j_target + w_energy * j_energy)


def _metrics(s, cells, w_energy):
    """KEYS from the five sums [..., 5] over `cells` cells per channel."""
    j_target, j_energy = -s[..., 4], s[..., 3] / (2 * cells)
    return dict(mse=(s[..., 0] + s[..., 1]) / (4 * cells), mse_wo_smoke=s[..., 0] / (3 * cells), n_l2=np.sqrt(s[..., 0]) / np.sqrt(s[..., 2]),
                J_target=j_target, J_energy=j_energy, J_total=j_target + w_energy * j_energy)


COMPARISONS = ('base', 'current', 'linear', 'nearest')


def score_super(pred, data, w_energy):
    """pred [B, T, 6, n, n] fp32 on the GPU (a cascade level), data [B, T, 6, N, N] fp32 or fp64 on pred's device (any strides), n == N or
    2 n == N. Returns {key: fp64 numpy [4, B]} for KEYS: row i is COMPARISONS[i] of multi_evaluate's super-resolution branch --
    base: pred at stride 2 n / N against data[..., ::2, ::2]; current: pred against data at stride N / n; linear / nearest: pred
    interpolated (bilinear with align_corners=False / nearest) to N x N against data. The reference's 64 is N / 2 here."""
    from wdno_amd import _lib
    from wdno_amd.ops import _p, _stream
    if not pred.is_cuda or pred.dtype != torch.float32 or pred.dim() != 5 or pred.shape[2] != 6 or pred.shape[3] != pred.shape[4]:
        raise RuntimeError(f'smoke score: pred must be a float32 [B, T, 6, n, n] tensor on the GPU, got {pred.dtype} {tuple(pred.shape)} on {pred.device}')
    pred = pred.detach().contiguous()
    B, T, _, n, _ = (int(v) for v in pred.shape)
    N = int(data.shape[-1])
    if not torch.is_tensor(data) or tuple(data.shape) != (B, T, 6, N, N) or N % 2 or N not in (n, 2 * n):
        raise ValueError(f'smoke score: data {tuple(data.shape)} against pred {tuple(pred.shape)}: [B, T, 6, N, N] with N = n or 2 n (even) is needed')
    table = _channel_table([data[:, :, c] for c in range(6)], (B, T, N, N), pred.device)
    with torch.cuda.device(pred.device):
        out = torch.empty(B, 4, 5, dtype=torch.float64, device=pred.device)
        _lib.check(_lib.load().wdno_smoke_score_super(_p(pred), table, _p(out), B, T, n, N, _stream()), 'wdno_smoke_score_super')
    s = out.cpu().numpy().transpose(1, 0, 2)                                  # [4, B, 5]
    cells = np.array([T * g * g for g in (N // 2, n, N, N)], dtype=np.float64).reshape(4, 1)
    return _metrics(s, cells, w_energy)


def control_channels(pred, density, velocity, ratio):
    """The six data channels of control mode. pred [B, T, 6, h, w] with the control interior already zeroed; density [B, T, 128, 128],
    velocity [B, T, 128, 128, 2] and ratio [B, 256] fp64 as smoke_solver.solve(frames=range(0, 256, 256 // T)) returns them."""
    B, T, _, h, w = pred.shape
    s, ft = density.shape[-1] // w, ratio.shape[1] // T
    return [density[:, :, ::s, ::s], velocity[:, :, ::s, ::s, 0], velocity[:, :, ::s, ::s, 1], pred[:, :, 3], pred[:, :, 4],
            ratio[:, ::ft, None, None].expand(B, T, h, w)]


def score_controls(pred, data, w_energy, geom=None, threads=None):
    """Control mode of multi_evaluate for pred, data [B, T, 6, nx, nx]: the initial density data[:, 0, 0] and the controls of pred with
    their interior zeroed (inference_2d.py:337, 388) are re-simulated, only the T frames the metrics read are written, and score() reads
    them in place. Returns score()'s dict."""
    from wdno_amd import smoke_solver
    if not pred.is_cuda:
        raise RuntimeError('smoke score: pred must live on the GPU (no CPU fallback on the hot path)')
    pred = pred.detach().to(torch.float32).clone()
    sp = int(data.shape[-1] / pred.shape[-1])
    pred[:, 0, 0] = data[:, 0, 0, ::sp, ::sp].to(pred.device, torch.float32)
    pred[:, :, 3:5, 8:56, 8:56] = 0
    T = int(pred.shape[1])
    density, _, velocity, ratio = smoke_solver.solve(pred[:, 0, 0], pred[:, :, 3], pred[:, :, 4], frames=range(0, smoke_solver.NUM_T, smoke_solver.NUM_T // T),
                                                     geom=geom, threads=threads)
    return score(pred, control_channels(pred, density, velocity, ratio), w_energy)
