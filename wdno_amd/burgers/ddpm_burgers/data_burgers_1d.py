"""Datasets of the 1-D Burgers task -- drop-in for burgers/ddpm_burgers/data_burgers_1d.py.

`get_wavelet_super_preprocess` turns the coefficient file of the offline transform
    {'coef': [level][N, 2, 4, h, w], 'shape', 'ori_shape'}
into U-Net inputs [N, C, 64, 64]: channels 0-3 the sub-bands of u, 4-7 those of f, zero-padded from 41 x 60 (8 more channels
with the nearest-upsampled next-coarser level for super-resolution models), and one condition channel that holds the 1-D DWT
of u(t=0) and u(t=T) in four horizontal stripes; everything divided by the per-channel rescaler. The condition channel needs
the physical u: IDWT of the packed coefficients, then a 1-D DWT of two rows -- both run on the GPU here (the reference used
pytorch_wavelets on whatever device the file was loaded to); the rest is indexing. Results come back on the device of the
input file, so `DiffusionDataset` / `DataLoader` behave as before.

`pack_burgers_gpu` packs a BATCH of such inputs from coefficient levels resident in HBM in one launch (csrc/pack_burgers.hip: the two
rows of u behind the condition channel are synthesised inside the launch), `pack_burgers_batch` is the same on tensors of any device;
wdno_amd.loader.ResidentSuperBurgersLoader feeds the super-resolution trainer with them.
"""
import math
import os
import random
import weakref

import torch
from torch import nn
from torch.utils.data import DataLoader, Dataset

from ddpm_burgers.model_utils import cycle
from ddpm_burgers.wavelet_utils import upsample_coef  # noqa: F401  (re-export)
from wave_trans import tensor_to_coef

_MAX_SAMPLES = 40000


def _nearest2(t):
    """nearest x2 in (t, x) of [N, l, nt, nx] (ddpm_burgers.wavelet_utils.upsample_coef): indexing only, any device"""
    return t.repeat_interleave(2, dim=-2).repeat_interleave(2, dim=-1)


def _gpu_chunks(n, chunk=2048):
    return [(a, min(n, a + chunk)) for a in range(0, n, chunk)]


def _condition_rows(w_uf, shape, ori_shape, mode, wave_type):
    """1-D DWT of u(t=0) and u(t=T) from packed coefficients [N, >=8, 64, 64]: -> (lo [N, 2, nx], hi [N, 2, nx]) on w_uf's device"""
    from wdno_amd import wavelets as W
    ifm = W.DWTInverse(mode=mode, wave=wave_type)
    xfm1d = W.DWT1DForward(J=1, mode=mode, wave=wave_type)
    dev = w_uf.device
    gpu = torch.device('cuda', torch.cuda.current_device())
    los, his = [], []
    for a, b in _gpu_chunks(w_uf.shape[0]):
        yl, yh = tensor_to_coef(w_uf[a:b, :8].to(gpu), shape)
        u = ifm((yl.contiguous(), [yh[0].contiguous()]))[:, 0, :ori_shape[-2], :ori_shape[-1]]
        lo, hi = xfm1d(u[:, [0, -1], :ori_shape[-1]].contiguous())
        los.append(lo.to(dev))
        his.append(hi[0].to(dev))
    return torch.cat(los), torch.cat(his)


def _pack_index(fine, coarse, rescaler, ori_shape, pad_t, pad_x, mode, wave_type, is_condition_u0, is_condition_uT):
    """The packing as index work on tensors of any device: fine [N, 2, 4, nt, nx], coarse [N, 2, 4, nt_c, nx_c] or None (base models),
    ori_shape = the level's (ori_t, ori_x) -> [N, C, pad_t, pad_x] / rescaler. The condition rows take _condition_rows' GPU route."""
    n, nt, nx = fine.size(0), fine.size(-2), fine.size(-1)
    w_uf = nn.functional.pad(fine.reshape(n, 8, nt, nx), (0, pad_x - nx, 0, pad_t - nt))                # [N, 8, pad, pad]
    out = w_uf
    if coarse is not None:
        sub = _nearest2(coarse.reshape(n, 8, coarse.size(-2), coarse.size(-1)))
        sub = nn.functional.pad(sub, (0, pad_x - sub.shape[-1], 0, pad_t - sub.shape[-2]))
        w_uf[:, :, nt, :] = w_uf[:, :, nt - 1, :]            # odd number of time coefficients: repeat the last one
        out = torch.cat((w_uf, sub), dim=1)
    if is_condition_u0 or is_condition_uT:
        lo, hi = _condition_rows(w_uf, (nt, nx), ori_shape, mode, wave_type)
        cond = torch.zeros_like(out[:, :1])
        rep = pad_t // 4
        if is_condition_u0:
            cond[:, 0, :rep, :nx] = lo[:, None, 0]
            cond[:, 0, rep:2 * rep, :nx] = hi[:, None, 0]
        if is_condition_uT:
            cond[:, 0, 2 * rep:3 * rep, :nx] = lo[:, None, 1]
            cond[:, 0, 3 * rep:4 * rep, :nx] = hi[:, None, 1]
        out = torch.cat((out, cond), dim=1)
    return out / rescaler


def level_ori_shape(ori_shape, lvl):
    return [math.ceil(ori_shape[0] / 2 ** lvl), math.ceil(ori_shape[1] / 2 ** lvl)]


def get_wavelet_super_preprocess(rescaler=70, is_super_model=False, N_downsample=0, mode='zero', wave_type='bior2.4',
                                 is_condition_u0=True, is_condition_uT=True):
    if rescaler is None:
        raise NotImplementedError('Should specify rescaler. If no rescaler is not used, specify 1.')

    def preprocess(db):
        lvl = N_downsample if is_super_model else 0
        data = db['coef']
        fine = data[lvl][:_MAX_SAMPLES]
        coarse = data[lvl + 1][:_MAX_SAMPLES] if is_super_model else None
        ori_shape = level_ori_shape(db['ori_shape'], lvl)
        pad_t = pad_x = int(64 / 2 ** lvl)
        out = _pack_index(fine, coarse, rescaler, ori_shape, pad_t, pad_x, mode, wave_type, is_condition_u0, is_condition_uT)
        return out, list(fine.shape[-2:]), ori_shape

    # (what a loader needs to pack the same batches itself: wdno_amd.loader.ResidentSuperBurgersLoader, DiffusionDataset's lazy x)
    preprocess.args = dict(rescaler=rescaler, is_super_model=is_super_model, N_downsample=N_downsample, mode=mode, wave_type=wave_type,
                           is_condition_u0=is_condition_u0, is_condition_uT=is_condition_uT)
    return preprocess


def _rescaler_vector(rescaler, c):
    r = torch.as_tensor(rescaler, dtype=torch.float32).reshape(-1)
    if r.numel() == 1:
        r = r.expand(c)
    if r.numel() != c:
        raise ValueError(f'rescaler has {r.numel()} entries, the state {c} channels')
    return r.contiguous()


def pack_burgers_batch(fine, coarse, rescaler, ori_shape, idx=None, pad_t=64, pad_x=64, mode='periodization', wave_type='bior2.4',
                       is_condition_u0=True, is_condition_uT=True):
    """get_wavelet_super_preprocess for a batch taken from coefficient levels held on one device: fine [N, 2, 4, nt, nx] (level l), coarse
    [N, 2, 4, nt_c, nx_c] (level l + 1; None: a base model), ori_shape = level l's field size; idx picks the samples of the batch (None: all, in
    order) -> [B, 8 + 8 has_low + has_cond, pad_t, pad_x] / rescaler. On CUDA tensors and periodization it is one launch of csrc/pack_burgers.hip
    (pack_burgers_gpu); otherwise the index formulation of the preprocess on the gathered samples. Both give the same bits in every channel,
    the condition channel included: the launch keeps the summation order of the transforms behind _condition_rows
    (tests/test_gpu_burgers_super_loader.py)."""
    if fine.is_cuda and mode in ('periodization', 'per'):
        return pack_burgers_gpu(fine, coarse, rescaler, ori_shape, idx, pad_t, pad_x, wave_type, is_condition_u0, is_condition_uT)
    if idx is not None:
        idx = torch.as_tensor(idx, dtype=torch.int64, device=fine.device)
        fine = fine.index_select(0, idx)
        coarse = None if coarse is None else coarse.index_select(0, idx)
    c = 8 + (8 if coarse is not None else 0) + (1 if (is_condition_u0 or is_condition_uT) else 0)
    r = _rescaler_vector(rescaler, c).to(fine.device).reshape(1, c, 1, 1)
    return _pack_index(fine, coarse, r, list(ori_shape), pad_t, pad_x, mode, wave_type, is_condition_u0, is_condition_uT)


_taps = {}


def pack_burgers_gpu(fine, coarse, rescaler, ori_shape, idx=None, pad_t=64, pad_x=64, wave_type='bior2.4', is_condition_u0=True,
                     is_condition_uT=True):
    """wdno_pack_burgers_state (csrc/pack_burgers.hip): the states of a batch in one launch from device-resident coefficient levels, periodization
    mode. Arguments as pack_burgers_batch; idx is an int64 device tensor [B]. The shape rules are the library's (include/wdno_hip.h)."""
    import ctypes as C
    from wdno_amd import _lib
    from wdno_amd.filters import filter_bank
    from wdno_amd.ops import _lib_, _p, _stream
    for t, name in ((fine, 'fine'), (coarse, 'coarse')):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError(f'wdno_amd pack_burgers_gpu: {name} must be a contiguous float32 tensor on the GPU')
    n, nt, nx = fine.shape[0], fine.shape[-2], fine.shape[-1]
    assert tuple(fine.shape[1:3]) == (2, 4) and (coarse is None or tuple(coarse.shape[:3]) == (n, 2, 4))
    nt_c, nx_c = (coarse.shape[-2], coarse.shape[-1]) if coarse is not None else (0, 0)
    c = 8 + (8 if coarse is not None else 0) + (1 if (is_condition_u0 or is_condition_uT) else 0)
    r = _rescaler_vector(rescaler, c).to(fine.device)
    taps = _taps.get(wave_type)
    if taps is None:
        taps = _taps[wave_type] = tuple((C.c_float * len(bank))(*[float(v) for v in bank]) for bank in filter_bank(wave_type))
    if idx is not None:
        idx = idx.to(device=fine.device, dtype=torch.int64).contiguous()
    b = n if idx is None else idx.numel()
    with torch.cuda.device(fine.device):
        out = torch.empty((b, c, pad_t, pad_x), device=fine.device, dtype=torch.float32)
        _lib.check(_lib_().wdno_pack_burgers_state(_p(fine), fine[0].numel(), _p(coarse), 0 if coarse is None else coarse[0].numel(), _p(idx), _p(r),
                                                   _p(out), b, nt, nx, nt_c, nx_c, pad_t, pad_x, int(ori_shape[0]), int(ori_shape[1]),
                                                   int(coarse is not None), int(bool(is_condition_u0)), int(bool(is_condition_uT)), *taps,
                                                   len(taps[0]), _stream()), 'pack_burgers_state')
    return out


def get_burgers_preprocess(rescaler=10, is_super_model_train=False, N_downsample=0, is_super_model_test=False, upsample_t=0, upsample_x=0):
    """Physical-space (non-wavelet) packing, data_burgers_1d.py:168-211: u, f zero-padded to 128 x 128 (times 2^upsample)."""
    if rescaler is None:
        raise NotImplementedError('Should specify rescaler. If no rescaler is not used, specify 1.')

    def preprocess(db):
        if is_super_model_test:
            super_nt, super_nx = db['f'].shape[-2], db['u'].shape[-1]
            assert super_nt / 80 / 2 ** upsample_t > 0
            st, sx = int(super_nt / 80 / 2 ** upsample_t), int(super_nx / 120 / 2 ** upsample_x)
            u, f = db['u'][:, ::st, ::sx], db['f'][:, ::st, ::sx]
        else:
            u, f = db['u'][:_MAX_SAMPLES], db['f'][:_MAX_SAMPLES]
        nt, nx = f.size(-2), f.size(-1)
        shape = u[..., ::2 ** N_downsample, ::2 ** N_downsample].shape[-2:]
        f = nn.functional.pad(f, (0, 128 * 2 ** upsample_x - nx, 0, 128 * 2 ** upsample_t - nt))
        u = nn.functional.pad(u, (0, 128 * 2 ** upsample_x - nx, 0, 128 * 2 ** upsample_t - 1 - nt))
        data = torch.stack((u, f), dim=1)
        if is_super_model_train:
            uf = data[:, :, ::2 ** N_downsample, ::2 ** N_downsample]
            uf_sub = _nearest2(data[:, :, ::2 ** (N_downsample + 1), ::2 ** (N_downsample + 1)])
            nt_sub = int(nt / 2 ** N_downsample)
            uf[:, :, nt_sub + 1, :] = uf[:, :, nt_sub, :]
            data = torch.cat((uf, uf_sub), dim=1)
        return data / rescaler, list(shape), list(shape)

    return preprocess


def get_wavelet_preprocess(rescaler=70, mode='zero', wave_type='bior2.4', is_condition_u0=True, is_condition_uT=True):
    """Multi-level (J = len(shape)) variant of the packer, data_burgers_1d.py:90-166. train_ddpm_burgers.py never selects it
    (it only appears as the default argument of DiffusionDataset); the single-level packer above is the WDNO path."""
    if rescaler is None:
        raise NotImplementedError('Should specify rescaler. If no rescaler is not used, specify 1.')

    def preprocess(db):
        raise NotImplementedError('multi-level coefficient datasets are not produced by wave_trans.py; use get_wavelet_super_preprocess')

    return preprocess


class _FileDict(dict):
    """A file's dictionary that can be referenced weakly and remembers the mtime it was read at"""
    mtime = None


_files = weakref.WeakValueDictionary()     # path -> the file's dictionary, for as long as a dataset holds it: the level datasets of one
                                           # coefficient file share one read, and nothing stays in host memory after the last of them is gone


def _read_file(fname):
    path = os.path.abspath(fname)
    mtime = os.path.getmtime(path)
    held = _files.get(path)
    if held is None or held.mtime != mtime:
        held = _FileDict(torch.load(path, weights_only=False))
        held.mtime = mtime
        _files[path] = held
    return held


class DiffusionDataset(Dataset):
    """x [N, C, pad, pad]: the packed tensor of the whole file, built by `preprocess` in the constructor. With the preprocess of a
    super-resolution level (get_wavelet_super_preprocess(is_super_model=True)) shape, ori_shape and the length come from the file's metadata
    and x is built on its first use (`x`, `ds[i]`) -- a loader that packs batches from the coefficient levels themselves
    (wdno_amd.loader.ResidentSuperBurgersLoader) never builds it. The first use must happen in the process that owns the dataset:
    DataLoader workers would each build a copy of their own."""

    def __init__(self, fname, preprocess=None):
        self.db = _read_file(fname) if isinstance(fname, str) else fname
        self.preprocess = preprocess or get_wavelet_preprocess()
        a = getattr(self.preprocess, 'args', None)
        if a is not None and a['is_super_model']:
            fine = self.db['coef'][a['N_downsample']]
            self._x, self._len = None, min(fine.shape[0], _MAX_SAMPLES)
            self.shape, self.ori_shape = list(fine.shape[-2:]), level_ori_shape(self.db['ori_shape'], a['N_downsample'])
        else:
            self._x, self.shape, self.ori_shape = self.preprocess(self.db)
            self._len = self._x.size(0)

    @property
    def x(self):
        if self._x is None:
            if torch.utils.data.get_worker_info() is not None:
                raise RuntimeError('DiffusionDataset: x of a super-resolution level is built on first use, and this is a DataLoader worker: '
                                   'touch `dataset.x` in the parent process before the workers start (SuperDataLoader does)')
            self._x = self.preprocess(self.db)[0]
        return self._x

    def __len__(self):
        return self._len

    def __getitem__(self, idx):
        return self.x[idx]

    def get(self, idx):
        return self.__getitem__(idx)

    def len(self):
        return self.__len__()


class SuperDataLoader:
    """One batch per iteration from a randomly chosen dataset of the list (super-resolution levels)."""

    def __init__(self, dataset, batch_size=1, shuffle=True, pin_memory=True, num_workers=1, seed=None):
        """seed (an extension): private shuffle / level-choice streams, e.g. base + 1000 * rank under data parallelism -- the
        reference's loader is not sharded by accelerate, and identically seeded ranks would draw identical batches."""
        self.dataset = dataset
        for ds in dataset:                # a level's packed tensor is built on first use: here, not once in every worker process
            getattr(ds, 'x', None)
        gens = [None if seed is None else torch.Generator().manual_seed(seed + i) for i in range(len(dataset))]
        self.dl = [cycle(DataLoader(ds, batch_size=batch_size, shuffle=shuffle, pin_memory=pin_memory, num_workers=num_workers, generator=g))
                   for ds, g in zip(dataset, gens)]
        self.num_batches = len(dataset) * ((len(dataset[0]) + batch_size - 1) // batch_size)
        self._rng = random if seed is None else random.Random(seed)

    def __iter__(self):
        yield next(self.dl[self._rng.randint(0, len(self.dl) - 1)])

    def __len__(self):
        return self.num_batches
