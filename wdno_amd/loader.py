"""Input pipelines that keep the host off a training step's critical path (VERDICT r5 missing #5).

The reference feeds both trainers through torch DataLoaders (burgers/ddpm_burgers/train_diffusion.py:93-101, smoke/ddpm/diffusion_2d.py:1146-1157):
the Burgers dataset is one packed host tensor indexed per sample, the smoke dataset does a `torch.load` of a pickle plus host-side packing PER
SAMPLE (data_2d.py:156-221). At 258 samples/s/GPU x 6.45 MB that is 1.7 GB/s of pickles per GPU and 13 GB/s per 8-GPU node. MI355X has 288 GB of
HBM: the whole training set (smoke: 20 000 simulations x 3.35 MB of raw coefficients = 67 GB; Burgers: 5.9 GB packed) fits beside the model, so

  * ResidentTensorLoader : a map-style dataset whose samples are rows of ONE tensor (DiffusionDataset.x) lives in HBM; a batch is an index gather.
  * ResidentSmokeLoader  : every simulation file is read ONCE (worker processes, pinned staging, in the order the first epoch needs them) into
                           resident stores of the RAW arrays, and every batch -- first epoch and after -- is packed on the GPU by
                           wdno_pack_smoke_state (csrc/pack.hip). From the second epoch on no host code touches the data.
  * ResidentSuperSmokeLoader : the same for the list of level datasets of a super-resolution smoke model (SuperDataLoader's contract: one batch of
                           one randomly chosen level per iteration): one set of stores per coefficient level, each file read once for all levels,
                           every two-level batch packed by wdno_pack_smoke_super_state.
  * ResidentSuperBurgersLoader : the same contract for the level datasets of the Burgers super-resolution model: the coefficient levels of the one
                           file live in HBM once each, every batch is one launch of wdno_pack_burgers_state (csrc/pack_burgers.hip), condition
                           channel included; the packed host tensors of the levels are never built.

The first two iterate like `DataLoader(dataset, batch_size, shuffle=True, drop_last=False)` under a DistributedSampler (rank-disjoint shards of a padded
per-epoch permutation, reshuffled every epoch by `set_epoch`), yield DEVICE tensors, and are what the drop-in Trainers use when
`Trainer.resident_data` is on and the data fits (TrainerCore.make_loader)."""
import math

import torch
from torch.utils.data import DataLoader, Dataset


SMOKE_SIM_BYTES = 4 * (5 * 8 * 18 * 34 * 34 + 4 * 34 * 34 + 2 * 18)      # raw arrays of one base-resolution simulation (bior1.3 / zero: [32, 64, 64] -> [18, 34, 34])


class _EpochOrder:
    """Index order of one rank for one epoch: torch.utils.data.DistributedSampler's rule (seeded permutation of range(n), padded by wrapping to a
    multiple of the world size, every world-th index from `rank` on); world = 1: a plain permutation."""

    def __init__(self, n, rank=0, world=1, shuffle=True, seed=0):
        self.n, self.rank, self.world, self.shuffle, self.seed, self.epoch = n, rank, world, shuffle, seed, 0

    def set_epoch(self, epoch):
        self.epoch = epoch

    def indices(self):
        if self.shuffle:
            g = torch.Generator().manual_seed(self.seed + self.epoch)
            idx = torch.randperm(self.n, generator=g).tolist()
        else:
            idx = list(range(self.n))
        if self.world > 1:
            total = math.ceil(self.n / self.world) * self.world
            idx += idx[:total - len(idx)]
            idx = idx[self.rank:total:self.world]
        return idx


class ResidentTensorLoader:
    """`DataLoader(dataset, batch_size, shuffle)` for a dataset that is one tensor (`dataset.x`, or the tensor itself): the tensor is moved to
    `device` once and a batch is `x[idx]` -- one gather launch, no worker processes, no pinned staging, no per-batch host-to-device copy."""

    def __init__(self, data, batch_size, device, shuffle=True, rank=0, world=1, seed=0):
        x = data.x if hasattr(data, 'x') else data
        self.x = x.to(device=device, dtype=torch.float32).contiguous()
        self.batch_size, self.device = batch_size, torch.device(device)
        self.sampler = _EpochOrder(self.x.shape[0], rank, world, shuffle, seed)          # (`.sampler.set_epoch`: trainer.cycle_loader)

    def __len__(self):
        return math.ceil(len(self.sampler.indices()) / self.batch_size)

    def __iter__(self):
        idx = torch.tensor(self.sampler.indices(), dtype=torch.int64).to(self.device)      # one small upload per epoch
        for k in range(0, idx.numel(), self.batch_size):
            yield self.x.index_select(0, idx[k:k + self.batch_size])


class _RawSims(Dataset):
    def __init__(self, ds, ids):
        self.ds, self.ids = ds, ids

    def __len__(self):
        return len(self.ids)

    def __getitem__(self, i):
        return self.ds.raw(self.ids[i])


class ResidentSmokeLoader:
    """`DataLoader(Smoke_wave(...), batch_size, shuffle)` with the data resident in HBM. Yields what the DataLoader's collate yields,
    `(state [B, 24, 42, 40, 40], shape, ori_shape, sim_id)`, with `state` already on the device.

    Stores (allocated once for `capacity` simulations, default all of them): coef [N, 5, 8, nt, nx, nx], init [N, 4, nx, nx], smokeout [N, 2, nt].
    A simulation enters the stores the first time an epoch's order reaches it: its file is read by a DataLoader worker (`torch.load` in another
    process, pinned hand-over), copied to its slot, and from then on it is only ever indexed. Files are requested in the order the epoch will use
    them, `prefetch` batches ahead of the consumer."""

    def __init__(self, dataset, batch_size, device, shuffle=True, rank=0, world=1, seed=0, num_workers=8, prefetch=4, rescaler=None):
        if getattr(dataset, 'is_super_model', False):
            raise ValueError('ResidentSmokeLoader serves the base-resolution dataset (the super-resolution levels pair two coefficient levels per sample)')
        self.ds, self.batch_size, self.device = dataset, batch_size, torch.device(device)
        self.sampler = _EpochOrder(len(dataset), rank, world, shuffle, seed)
        self.num_workers, self.prefetch = num_workers, prefetch
        self.rescaler = (dataset.RESCALER if rescaler is None else rescaler).reshape(-1).to(self.device, torch.float32)
        self.slot = {}                    # sim id -> row of the stores
        self.coef = self.init = self.so = None
        self.shape = self.ori_shape = None

    def _alloc(self, coef, init, so):
        n = len(self.ds)
        self.coef = torch.empty((n, *coef.shape), device=self.device, dtype=torch.float32)
        self.init = torch.empty((n, *init.shape), device=self.device, dtype=torch.float32)
        self.so = torch.empty((n, *so.shape), device=self.device, dtype=torch.float32)

    def resident_bytes(self):
        return 0 if self.coef is None else 4 * (self.coef.numel() + self.init.numel() + self.so.numel())

    def __len__(self):
        return math.ceil(len(self.sampler.indices()) / self.batch_size)

    def __iter__(self):
        from ddpm.data_2d import pack_smoke_gpu
        order = self.sampler.indices()
        seen, missing = set(self.slot), []
        for i in order:
            if i not in seen:
                seen.add(i)
                missing.append(i)
        feed = None
        if missing:           # files not resident yet, in the order this epoch meets them; workers run `prefetch` batches ahead
            feed = iter(DataLoader(_RawSims(self.ds, missing), batch_size=None, shuffle=False, num_workers=self.num_workers, pin_memory=True,
                                   prefetch_factor=(max(2, self.prefetch * self.batch_size // max(1, self.num_workers)) if self.num_workers else None)))
        for k in range(0, len(order), self.batch_size):
            ids = order[k:k + self.batch_size]
            for i in ids:
                if i not in self.slot:
                    coef, init, so = next(feed)
                    if self.coef is None:
                        self._alloc(coef, init, so)
                    s = len(self.slot)
                    self.coef[s].copy_(coef, non_blocking=True)          # (pinned source: an asynchronous copy on the launch stream, ahead of the pack)
                    self.init[s].copy_(init, non_blocking=True)
                    self.so[s].copy_(so, non_blocking=True)
                    self.slot[i] = s
            idx = torch.tensor([self.slot[i] for i in ids], dtype=torch.int64).to(self.device, non_blocking=True)
            state = pack_smoke_gpu(self.coef, self.init, self.so, self.rescaler, idx)
            shape = list(self.coef.shape[-3:])
            yield state, shape, None, torch.tensor(ids)


class _RawLevelSims(Dataset):
    def __init__(self, ds, ids, n_levels):
        self.ds, self.ids, self.n_levels = ds, ids, n_levels

    def __len__(self):
        return len(self.ids)

    def __getitem__(self, i):
        return self.ds.raw_levels(self.ids[i], self.n_levels)


class ResidentSuperSmokeLoader:
    """`SuperDataLoader([Smoke_wave(..., is_super_model=True, N_downsample=i) for i < N], batch_size)` with the data resident in HBM: every
    `__iter__` yields ONE batch of one randomly chosen level, `(state [B, pad_t, 82, pad_x, pad_x], shape, ori_shape, sim_id)` with `state` on the
    device, pad_t / pad_x as Smoke_wave.__getitem__ sets them for the level (24 / 2^i and 40 for time, 24 and 40 / 2^i for space).

    Stores: one set (coef, init, smokeout) per coefficient level 0 .. N; level i + 1 is dataset i's coarse level and dataset i + 1's fine level, so
    nothing is held twice. A simulation's file is read ONCE, for all levels (Smoke_wave.raw_levels; the reference reads it per level's dataset and
    per sample), by DataLoader workers with pinned hand-over, in the order the levels' current epochs will need the files; a batch whose
    simulations are not all resident yet takes files from that stream until they are. Every batch is packed by one launch of
    wdno_pack_smoke_super_state (csrc/pack.hip) with an index list.

    Each level has its own _EpochOrder (seed `order_seed` + level, sharded by rank / world like a DistributedSampler), cursor and epoch counter;
    the short last batch of a level's epoch is kept. `seed` (None: the global `random`) makes the level choice a private random.Random(seed), as
    SuperDataLoader's does; ranks that are given the same `seed` draw the same level at every step and so walk each level's epochs in lockstep."""

    def __init__(self, datasets, batch_size, device, shuffle=True, rank=0, world=1, seed=None, order_seed=0, num_workers=8, prefetch=4):
        import random
        datasets = list(datasets)
        if not datasets or not all(getattr(d, 'is_super_model', False) and hasattr(d, 'raw_levels') for d in datasets):
            raise ValueError('ResidentSuperSmokeLoader serves a list of super-resolution Smoke_wave datasets (the base dataset: ResidentSmokeLoader)')
        if [d.N_downsample for d in datasets] != list(range(len(datasets))) or len({(d.path(0), len(d)) for d in datasets}) != 1:
            raise ValueError('ResidentSuperSmokeLoader: the datasets must be the levels 0 .. N - 1 of one set of files')
        self.ds, self.batch_size, self.device = datasets, batch_size, torch.device(device)
        self.kind = 'space' if datasets[0].downsample_type == 'space' else 'time'
        self.n_levels = len(datasets) + 1                          # coefficient levels held: dataset i pairs level i with level i + 1
        self.samplers = [_EpochOrder(len(datasets[0]), rank, world, shuffle, order_seed + lvl) for lvl in range(len(datasets))]
        self.epoch = [0] * len(datasets)
        self._order = [None] * len(datasets)
        self._cursor = [0] * len(datasets)
        self._rng = random if seed is None else random.Random(seed)
        self.num_workers, self.prefetch = num_workers, prefetch
        self.rescaler = [d.RESCALER.reshape(-1).to(self.device, torch.float32) for d in datasets]
        self.slot = {}                    # sim id -> row of the stores (the same row at every level)
        self.coef = self.init = self.so = None
        self._feeds, self._pending = [], set()

    def pads(self, lvl):
        return (24 // 2 ** lvl, 40) if self.kind == 'time' else (24, 40 // 2 ** lvl)

    def resident_bytes(self):
        return 0 if self.coef is None else 4 * sum(t.numel() for store in (self.coef, self.init, self.so) for t in store)

    def __len__(self):
        return len(self.ds) * math.ceil(len(self.samplers[0].indices()) / self.batch_size)

    def _open_feed(self):
        """Workers on every file the levels' current epochs still need and no stream has queued, batch by batch across the levels."""
        rest = [o[c:] if o is not None else [] for o, c in zip(self._order, self._cursor)]
        ids, seen = [], set(self.slot) | self._pending
        for k in range(0, max(len(o) for o in rest), self.batch_size):
            for o in rest:
                for i in o[k:k + self.batch_size]:
                    if i not in seen:
                        seen.add(i)
                        ids.append(i)
        self._pending.update(ids)
        dl = DataLoader(_RawLevelSims(self.ds[0], ids, self.n_levels), batch_size=None, shuffle=False, num_workers=self.num_workers,
                        pin_memory=self.device.type == 'cuda',
                        prefetch_factor=(max(2, self.prefetch * self.batch_size // max(1, self.num_workers)) if self.num_workers else None))
        self._feeds.append(zip(ids, dl))

    def _store(self, sim, levels):
        if self.coef is None:
            n = len(self.ds[0])
            self.coef, self.init, self.so = ([torch.empty((n, *lv[k].shape), device=self.device, dtype=torch.float32) for lv in levels] for k in range(3))
        s = len(self.slot)
        for lvl, (coef, init, so) in enumerate(levels):
            self.coef[lvl][s].copy_(coef, non_blocking=True)          # (pinned source: asynchronous copies on the launch stream, ahead of the pack)
            self.init[lvl][s].copy_(init, non_blocking=True)
            self.so[lvl][s].copy_(so, non_blocking=True)
        self.slot[sim] = s
        self._pending.discard(sim)

    def _fetch(self, sim):
        if sim not in self._pending:
            self._open_feed()
        while sim not in self.slot:
            got = next(self._feeds[0], None)
            if got is None:
                self._feeds.pop(0)
            else:
                self._store(*got)

    def __iter__(self):
        from ddpm.data_2d import pack_smoke_super_batch
        lvl = self._rng.randint(0, len(self.ds) - 1)
        if self._order[lvl] is None or self._cursor[lvl] >= len(self._order[lvl]):
            if self._order[lvl] is not None:
                self.epoch[lvl] += 1
            self.samplers[lvl].set_epoch(self.epoch[lvl])
            self._order[lvl], self._cursor[lvl] = self.samplers[lvl].indices(), 0
        ids = self._order[lvl][self._cursor[lvl]:self._cursor[lvl] + self.batch_size]
        for i in ids:
            if i not in self.slot:
                self._fetch(i)
        self._cursor[lvl] += len(ids)
        idx = torch.tensor([self.slot[i] for i in ids], dtype=torch.int64).to(self.device, non_blocking=True)
        pad_t, pad_x = self.pads(lvl)
        state = pack_smoke_super_batch(self.coef[lvl], self.coef[lvl + 1], self.init[lvl], self.so[lvl], self.rescaler[lvl], self.kind, idx, pad_t, pad_x)
        yield state, list(self.coef[lvl].shape[-3:]), None, torch.tensor(ids)


class ResidentSuperBurgersLoader:
    """`SuperDataLoader([DiffusionDataset(file, get_wavelet_super_preprocess(is_super_model=True, N_downsample=i)) for i < N], batch_size)` with the
    coefficient levels resident in HBM: every `__iter__` yields ONE batch of one randomly chosen level, a device tensor [B, C, pad, pad] with
    pad = 64 / 2^level, packed by one launch of wdno_pack_burgers_state (csrc/pack_burgers.hip) with an index list. The datasets' packed host
    tensors (DiffusionDataset.x: 11.1 + 2.8 + 0.7 GB for 40 000 samples and three levels) are never built.

    Levels 0 .. N are uploaded once each at construction; level i + 1 is dataset i's coarse level and dataset i + 1's fine level. Each level has
    its own _EpochOrder (seed `order_seed` + level, sharded by rank / world like a DistributedSampler), cursor and epoch counter; the short last
    batch of a level's epoch is kept. `seed` (None: the global `random`) makes the level choice a private random.Random(seed), as
    SuperDataLoader's does. device='cpu' packs the same batches through the index formulation (ddpm_burgers.data_burgers_1d.pack_burgers_batch)."""

    def __init__(self, datasets, batch_size, device, shuffle=True, rank=0, world=1, seed=None, order_seed=0):
        import random
        from ddpm_burgers.data_burgers_1d import _rescaler_vector, level_ori_shape
        levels = self.levels_of(datasets)
        self.ds, self.batch_size, self.device = list(datasets), batch_size, torch.device(device)
        self.args = [d.preprocess.args for d in self.ds]
        self.coef = [lv.to(device=self.device, dtype=torch.float32).contiguous() for lv in levels]
        self.ori_shape = [level_ori_shape(self.ds[0].db['ori_shape'], lvl) for lvl in range(len(self.ds))]
        c = 16 + (1 if (self.args[0]['is_condition_u0'] or self.args[0]['is_condition_uT']) else 0)
        self.rescaler = [_rescaler_vector(a['rescaler'], c).to(self.device) for a in self.args]          # (uploaded once, not per batch)
        n = self.coef[0].shape[0]
        self.samplers = [_EpochOrder(n, rank, world, shuffle, order_seed + lvl) for lvl in range(len(self.ds))]
        self.epoch = [0] * len(self.ds)
        self._order = [None] * len(self.ds)
        self._order_dev = [None] * len(self.ds)          # the epoch's order on the device: one small upload per level and epoch, none per batch
        self._cursor = [0] * len(self.ds)
        self._rng = random if seed is None else random.Random(seed)

    @staticmethod
    def levels_of(datasets):
        """The coefficient levels 0 .. N of a list of level datasets (host tensors, cut to the datasets' length), or ValueError unless the list is
        the levels 0 .. N - 1 of one file with one set of condition flags."""
        datasets = list(datasets)
        args = [getattr(getattr(d, 'preprocess', None), 'args', None) for d in datasets]
        if not datasets or not all(a is not None and a['is_super_model'] for a in args):
            raise ValueError('ResidentSuperBurgersLoader serves a list of DiffusionDatasets built with get_wavelet_super_preprocess(is_super_model=True)')
        if [a['N_downsample'] for a in args] != list(range(len(datasets))) or any(d.db is not datasets[0].db for d in datasets):
            raise ValueError('ResidentSuperBurgersLoader: the datasets must be the levels 0 .. N - 1 of one coefficient file')
        if len({(a['mode'], a['wave_type'], bool(a['is_condition_u0']), bool(a['is_condition_uT'])) for a in args}) != 1:
            raise ValueError('ResidentSuperBurgersLoader: the levels must share the wavelet, the mode and the condition flags')
        coef = datasets[0].db['coef']
        if len(coef) < len(datasets) + 1:
            raise ValueError(f'ResidentSuperBurgersLoader: {len(datasets)} levels need {len(datasets) + 1} coefficient levels, the file has {len(coef)}')
        return [coef[lvl][:len(datasets[0])] for lvl in range(len(datasets) + 1)]

    def resident_bytes(self):
        return 4 * sum(t.numel() for t in self.coef)

    def __len__(self):
        return len(self.ds) * math.ceil(len(self.samplers[0].indices()) / self.batch_size)

    def __iter__(self):
        from ddpm_burgers.data_burgers_1d import pack_burgers_batch
        lvl = self._rng.randint(0, len(self.ds) - 1)
        if self._order[lvl] is None or self._cursor[lvl] >= len(self._order[lvl]):
            if self._order[lvl] is not None:
                self.epoch[lvl] += 1
            self.samplers[lvl].set_epoch(self.epoch[lvl])
            self._order[lvl], self._cursor[lvl] = self.samplers[lvl].indices(), 0
            self._order_dev[lvl] = torch.tensor(self._order[lvl], dtype=torch.int64).to(self.device)
        k = self._cursor[lvl]
        ids = self._order[lvl][k:k + self.batch_size]
        idx = self._order_dev[lvl][k:k + self.batch_size]
        self._cursor[lvl] += len(ids)
        self.last_ids = (lvl, ids)                          # (tests / diagnostics: SuperDataLoader's batches carry no sample ids either)
        a, pad = self.args[lvl], 64 // 2 ** lvl
        yield pack_burgers_batch(self.coef[lvl], self.coef[lvl + 1], self.rescaler[lvl], self.ori_shape[lvl], idx, pad, pad, a['mode'], a['wave_type'],
                                 a['is_condition_u0'], a['is_condition_uT'])
