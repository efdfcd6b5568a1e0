"""Device-resident sample pool, epoch plan and the loader that turns both into batches with one kernel launch each.

The reference decodes, augments and ships every sample every epoch on 2-4 loader processes (the host
loader bounds real data well below what the training step consumes).  A sample is a 256 x 256 tile: 4 image bands, a mask
and a land-use map, 384 KiB as uint8 — 10^5 samples are 39 GB and fit in HBM several times over.  So every shard is decoded
once (``shards.read_shard``), the split stays resident as uint8 (``DevicePool``), the host draws one small plan per epoch
(``epoch_plan``: sample order and augmentation parameters) and ``PoolLoader`` makes every batch with one launch of the
gather kernel (csrc/pool.hip), if asked straight into the tensors a captured training step reads
(``HipTrainer.static_batch()``).

The reference's training configurations add extra shard sets to the main one (``pattern_extra`` / ``batch_size_extra``:
every batch is some main samples followed by a fixed number of each extra set, the shorter sets cycling).  Those are
several pools, one plan (``combined_plan``) and ``CombinedPoolLoader``, whose batches are still one launch each of the
same kernel: both loaders are one implementation (``_GatherLoader``), and a single pool is its one-source case.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from .distmap import distmaps_on_device
from .shards import read_shard, shard_len
from .synthetic import MEAN, STD


def _device_or_none(device):
    if device is not None:
        return torch.device(device)
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None


class DevicePool:
    """One split, contiguous: ``images`` uint8 [N,H,W,4], ``masks`` / ``lu`` uint8 [N,H,W], ``sums`` [N] (the exact sum
    of the 4*H*W bytes of every image: what RandomBrightnessContrast(brightness_by_max=False) needs, invariant under flips
    and turns, so computed once at decode time) and the host list ``stats`` of ``{"file", "frac"}`` dicts.

    With a HIP device the arrays are device tensors (``sums`` travels as the int64 bit pattern of the uint64 values; they
    stay below 2^63) filled through pinned host memory, one shard at a time.  Without one the pool keeps numpy arrays
    (``sums`` uint64), so shard handling can be set up and inspected anywhere; making batches needs the device."""

    def __init__(self, shards: Sequence, device=None, max_resident_bytes: Optional[int] = None, workers: int = 8):
        shards = [str(s) for s in shards]
        if not shards:
            raise ValueError("DevicePool: no shards")
        self.shards = shards
        self.device = dev = _device_or_none(device)
        on_gpu = dev is not None and dev.type == "cuda"
        if max_resident_bytes is None and on_gpu:
            max_resident_bytes = torch.cuda.mem_get_info(dev)[0] // 2
        alloc = None
        if on_gpu:      # decode into pinned memory: the upload is then one DMA per array
            def alloc(shape, dtype):
                return torch.empty(shape, dtype=torch.uint8, pin_memory=True).numpy()
        first = read_shard(shards[0], alloc=alloc, workers=workers)
        counts = [len(first["keys"])] + [shard_len(s) for s in shards[1:]]
        N = int(sum(counts))
        H, W = first["masks"].shape[1:]
        self.n, self.height, self.width = N, int(H), int(W)
        need = N * (H * W * 6 + 8)
        if max_resident_bytes is not None and need > max_resident_bytes:
            raise ValueError(f"DevicePool: {N} samples of {H}x{W} need {need} bytes resident, max_resident_bytes is "
                             f"{int(max_resident_bytes)} (streaming a split that does not fit is not supported)")
        if on_gpu:
            self.images = torch.empty((N, H, W, 4), dtype=torch.uint8, device=dev)
            self.masks = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
            self.lu = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
            self.sums = torch.empty(N, dtype=torch.int64, device=dev)
            self.device = self.images.device        # (with its index)
        else:
            self.images, self.masks = np.empty((N, H, W, 4), np.uint8), np.empty((N, H, W), np.uint8)
            self.lu, self.sums = np.empty((N, H, W), np.uint8), np.empty(N, np.uint64)
        self.stats = []
        at = 0
        for i, path in enumerate(shards):
            part = first if i == 0 else read_shard(path, alloc=alloc, workers=workers)
            n = len(part["keys"])
            if part["masks"].shape[1:] != (H, W):
                raise ValueError(f"{path}: tiles are {part['masks'].shape[1]}x{part['masks'].shape[2]}, "
                                 f"those of {shards[0]} are {H}x{W}")
            if n != counts[i]:
                raise ValueError(f"{path}: {n} samples decoded, {counts[i]} listed")
            if on_gpu:
                for name in ("images", "masks", "lu"):
                    getattr(self, name)[at:at + n].copy_(torch.from_numpy(part[name]), non_blocking=True)
                self.sums[at:at + n].copy_(torch.from_numpy(part["sums"].view(np.int64)))
                torch.cuda.current_stream(dev).synchronize()      # the pinned staging arrays are released after this
            else:
                for name in ("images", "masks", "lu", "sums"):
                    getattr(self, name)[at:at + n] = part[name]
            self.stats.extend(part["stats"])
            at += n
            first = None if i == 0 else first

    @classmethod
    def from_rasters(cls, items, tile_size: int = 256, source_dim: int = 2048, select="dead", masks: str = "keep",
                     device=None, max_resident_bytes: Optional[int] = None):
        """A pool filled straight from ortho rasters instead of shards (``data/rasters.py`` states the contract, the
        array arithmetic of the reference's scripts/createdataset.py).  ``items`` yields ``(key, rgbn uint8 [4,h,w], mask
        uint8 [h,w] | None, lu uint8 [h,w] | None)`` with h, w <= ``source_dim``; a field may also be a path that PIL opens,
        and mask / lu a ``PolygonSet`` in the raster's pixel coordinates (``data/polygons.py``), which is burnt on the
        device into its slot of the staged raster instead of being uploaded (on the host: ``rasterize_host``).
        Every raster is zero-padded to ``source_dim`` and cut into ``tile_size`` sub-tiles named ``f"{key}_{i:03}"``.
        ``select``: ``"dead"`` (sub-tiles whose rounded dead-pixel percentage is > 0), ``"valid"`` (every non-blank one)
        or a callable ``(names, census) -> bool[n]``; blank sub-tiles (min == max over the four bands) are never taken.
        ``masks="zero"`` writes zero masks (the reference's random set) and reports ``frac`` 0.0.

        The result is an ordinary pool: the same attributes, ``stats = [{"file": name, "frac": percentage}]`` and
        ``shards = []``.  With a HIP device every raster is one uint8 upload through pinned memory, one census launch
        (csrc/raster_cut.hip), one read-back of n x 128 bytes, the selection on the host and one cut launch into the
        pool's next rows.  The pool's tensors double when they are full and are trimmed to size at the end; before any
        growth the rows then needed are checked against ``max_resident_bytes`` (default: half of the free device memory)
        and the constructor's ``ValueError`` is raised.  Peak device memory: while a growth or the final trim copies,
        the old and the new tensors live side by side, at most three times the final pool's ``nbytes``, plus one staged
        raster (6 * source_dim^2 bytes).  Without a device the numpy contract fills a host pool."""
        from .rasters import pool_from_rasters
        return pool_from_rasters(items, tile_size, source_dim, select, masks, device, max_resident_bytes)

    def __len__(self):
        return self.n

    @property
    def on_device(self) -> bool:
        return isinstance(self.images, torch.Tensor)

    @property
    def nbytes(self) -> int:
        return self.n * (self.height * self.width * 6 + 8)


def epoch_plan(n: int, batch_size: int, epoch: int, seed: int, train: bool, square: bool = True, stream: Sequence = ()):
    """The whole epoch on the host: (idx int32 [M], geo int32 [M,2], bc float32 [M,2]) with M = (n // batch_size) *
    batch_size — the last partial batch is dropped, as by the reference's ``.batched(bs, partial=False)``.
    train: idx is the head of a permutation of n from ``np.random.default_rng([seed, epoch])`` and the augmentation draws
    are ``draw_train_params`` on the same generator; on non-square tiles a drawn turn k becomes ``k & 2`` (0 or a half
    turn; the generator's stream does not depend on the tile shape).  Otherwise idx is ``arange``, geo zeros and bc
    (1, 0).  Deterministic in (seed, epoch).  ``stream``: further integers of the generator's seed,
    ``default_rng([seed, epoch, *stream])`` — independent draws for the same (seed, epoch), as ``combined_plan`` needs them
    for its extra sources and their cycles."""
    from .deadtreedata import draw_train_params
    if batch_size < 1:
        raise ValueError(f"batch_size {batch_size}")
    m = (n // batch_size) * batch_size
    if not train:
        return (torch.arange(m, dtype=torch.int32), torch.zeros((m, 2), dtype=torch.int32),
                torch.tensor([1.0, 0.0]).repeat(m, 1))
    rng = np.random.default_rng([int(seed), int(epoch), *(int(v) for v in stream)])
    idx = torch.from_numpy(rng.permutation(n)[:m].astype(np.int32))
    if m == 0:
        return idx, torch.zeros((0, 2), dtype=torch.int32), torch.zeros((0, 2), dtype=torch.float32)
    geo, bc = draw_train_params(m, rng)
    if not square:
        geo[:, 1] &= 2
    return idx, geo, bc


def combined_plan(ns: Sequence[int], batch_sizes: Sequence[int], epoch: int, seed: int, train: bool, square: bool = True):
    """One epoch over several sources, the reference's ``CombinedLoader(..., "max_size_cycle")`` over loaders batched
    with ``partial=False`` (deadtreedata.py:348-395): source j has ``len_j = ns[j] // batch_sizes[j]`` batches, the epoch
    ``L = max(len_j)``, and a source that runs out starts over.  Returns ``(L, src int32 [M], idx int32 [M], geo int32
    [M,2], bc float32 [M,2])`` on the host, ``M = L * sum(batch_sizes)``: batch k is rows ``[k*B, (k+1)*B)``, in it
    ``batch_sizes[0]`` rows of source 0, then those of source 1, and so on.

    Source j at batch k is in cycle ``c = k // len_j`` at position ``p = k % len_j``; its rows are rows ``[p*bs_j,
    (p+1)*bs_j)`` of ``epoch_plan(ns[j], bs_j, epoch, seed, train, square, stream=S)`` with ``S = ()`` for (j, c) == (0, 0)
    and ``S = (j, c)`` otherwise: the main part of the first ``len_0`` batches is a plain ``PoolLoader`` epoch, every cycle
    the head of a fresh permutation.  Without ``train`` every cycle is ``arange`` with neutral parameters.  A source too
    small for one batch raises ``ValueError`` (there is nothing to cycle)."""
    ns, batch_sizes = [int(n) for n in ns], [int(b) for b in batch_sizes]
    if not ns or len(ns) != len(batch_sizes):
        raise ValueError(f"combined_plan: {len(ns)} sources, {len(batch_sizes)} batch sizes")
    if min(batch_sizes) < 1:
        raise ValueError(f"combined_plan: batch sizes {batch_sizes}")
    lens = [n // b for n, b in zip(ns, batch_sizes)]
    for j, (n, b) in enumerate(zip(ns, batch_sizes)):
        if lens[j] == 0:
            raise ValueError(f"combined_plan: source {j} holds {n} samples, fewer than its batch size {b}")
    L, B = max(lens), sum(batch_sizes)
    src = torch.empty((L, B), dtype=torch.int32)
    idx = torch.empty((L, B), dtype=torch.int32)
    geo = torch.empty((L, B, 2), dtype=torch.int32)
    bc = torch.empty((L, B, 2), dtype=torch.float32)
    at = 0
    for j, (n, b, ln) in enumerate(zip(ns, batch_sizes, lens)):
        src[:, at:at + b] = j
        for c in range(-(-L // ln)):
            stream = () if (j, c) == (0, 0) else (j, c)
            k0, k1 = c * ln, min((c + 1) * ln, L)
            for dst, part in zip((idx, geo, bc), epoch_plan(n, b, epoch, seed, train, square, stream=stream)):
                dst[k0:k1, at:at + b] = part[:(k1 - k0) * b].reshape((k1 - k0, b) + tuple(part.shape[1:]))
        at += b
    return L, src.reshape(-1), idx.reshape(-1), geo.reshape(-1, 2), bc.reshape(-1, 2)


class CombinedBatch(dict):
    """``{"main": (...), "extra_0": (...), ...}`` of the reference's five-tuples whose tensors are views of ONE contiguous
    tensor per field; ``combined`` is the five-tuple of those whole tensors (stats concatenated in key order) — what
    ``create_combined_batch`` would ``torch.cat`` together, and what it hands back instead."""

    def __init__(self, combined, batch_sizes: Sequence[int]):
        super().__init__()
        img, mask, dist, lu, stats = combined
        self.combined = (img, mask, dist, lu, stats)
        at = 0
        for j, b in enumerate(batch_sizes):
            part = slice(at, at + b)
            self["main" if j == 0 else f"extra_{j - 1}"] = (
                img[part], mask[part], None if dist is None else dist[part], None if lu is None else lu[part],
                stats[part])
            at += b
        if at != img.shape[0]:
            raise ValueError(f"CombinedBatch: batch sizes {list(batch_sizes)} for {img.shape[0]} samples")


class _GatherLoader:
    """What ``PoolLoader`` and ``CombinedPoolLoader`` are: the batches of one or several ``DevicePool``s, each made by
    one ``ops.pool_gather_combined`` launch on slices of the epoch's host plan (``_host_plan``), which is uploaded once per
    epoch; no host synchronisation and no host-to-device copy per batch.  ``classes == 2`` merges mask labels above 1
    into 1.  ``distmap``: attach ``distmaps_on_device`` maps, computed once on the whole batch (False: ``None``;
    ``HipTrainer`` computes them itself when a boundary loss needs them).

    ``trainer``: once ``trainer.static_batch()`` exists and its image and mask buffers have this loader's shapes, the
    gather writes into THOSE tensors and yields them, so the captured step finds its input in place; such batches are
    overwritten by the next one.  Before that (and without a trainer) every batch is a fresh set of tensors.

    Every ``__iter__`` starts the next epoch (0, 1, 2, ...), so a plain ``for batch in loader`` per epoch reshuffles;
    ``set_epoch(e)`` makes the next iteration epoch e.  The kernel's error flag (never raised by a plan of ``epoch_plan``
    or ``combined_plan``) is read once, after the last batch of an epoch."""

    def __init__(self, pools: Sequence[DevicePool], batch_sizes: Sequence[int], train: bool = False, in_channels: int = 3,
                 classes: int = 2, seed: int = 0, distmap: bool = True, trainer=None, mean=MEAN, std=STD):
        from .._lib import POOL_MAX_SOURCES
        who = type(self).__name__
        pools, batch_sizes = list(pools), [int(b) for b in batch_sizes]
        if not pools or len(pools) != len(batch_sizes):
            raise ValueError(f"{who}: {len(pools)} pools, {len(batch_sizes)} batch sizes")
        if len(pools) > POOL_MAX_SOURCES:
            raise ValueError(f"{who}: at most {POOL_MAX_SOURCES} pools, not {len(pools)}")
        if not all(p.on_device for p in pools):
            raise RuntimeError(f"{who} runs the HIP gather kernel on device-resident pools: no HIP device, no CPU fallback")
        if not 1 <= in_channels <= 4:
            raise ValueError(f"in_channels {in_channels}: the pool holds 4 bands")
        first = pools[0]
        for j, p in enumerate(pools):
            if (p.height, p.width) != (first.height, first.width) or p.device != first.device:
                raise ValueError(f"{who}: pool {j} holds {p.height}x{p.width} tiles on {p.device}, pool 0 "
                                 f"{first.height}x{first.width} on {first.device}")
        self.pools, self.batch_sizes, self.train = pools, batch_sizes, bool(train)
        self.batch_size = sum(batch_sizes)
        self.in_channels, self.classes, self.seed = int(in_channels), int(classes), int(seed)
        self.distmap, self.trainer = bool(distmap), trainer
        self.mean, self.std = tuple(mean), tuple(std)
        self.epoch = None            # the epoch of the running / last iteration
        self._next_epoch = 0
        self._eval_plan = None
        self._sources = [(p.images, p.masks, p.lu, p.sums) for p in pools]
        self._err = torch.zeros(1, dtype=torch.int32, device=first.device)

    def set_epoch(self, epoch: int):
        self._next_epoch = int(epoch)

    def __len__(self):
        raise NotImplementedError

    def _host_plan(self, epoch: int):
        """``(src, idx, geo, bc)`` of ``epoch`` on the host; src is None with one pool (every row is pool 0)"""
        raise NotImplementedError

    def _batch(self, item):
        """the yielded form of the five-tuple of whole tensors"""
        raise NotImplementedError

    def _static_out(self):
        sb = self.trainer.static_batch() if self.trainer is not None else None
        if sb is None:
            return None
        img, mask = sb[0], sb[1]
        p, dev = self.pools[0], self.pools[0].device
        ok = (tuple(img.shape) == (self.batch_size, self.in_channels, p.height, p.width) and img.dtype == torch.float32
              and tuple(mask.shape) == (self.batch_size, p.height, p.width) and mask.dtype == torch.int64
              and img.is_contiguous() and mask.is_contiguous() and img.device == dev and mask.device == dev)
        return (img, mask) if ok else None

    def __iter__(self):
        from .. import ops
        p, bs = self.pools[0], self.batch_size
        self.epoch = epoch = self._next_epoch
        self._next_epoch = epoch + 1
        if self.train or self._eval_plan is None:
            host = self._host_plan(epoch)
            dev_plan = tuple(None if t is None else t.to(p.device, non_blocking=True) for t in host)
            if not self.train:
                self._eval_plan = (host, dev_plan)
        else:
            host, dev_plan = self._eval_plan
        order = host[1].tolist()
        which = [0] * len(order) if host[0] is None else host[0].tolist()
        src, idx, geo, bc = dev_plan
        for k in range(len(self)):
            lo, hi = k * bs, (k + 1) * bs
            static = self._static_out()
            out = None
            if static is not None:      # lu is not an input of the step: it gets a tensor of its own
                out = (static[0], static[1], torch.empty((bs, p.height, p.width), dtype=torch.int64, device=p.device))
            img, mask, lu, _ = ops.pool_gather_combined(self._sources, None if src is None else src[lo:hi], idx[lo:hi],
                                                        geo[lo:hi], bc[lo:hi], self.mean, self.std, self.in_channels,
                                                        self.classes == 2, out=out, err=self._err)
            dist = distmaps_on_device(mask, self.classes) if self.distmap else None
            stats = [self.pools[j].stats[i] for j, i in zip(which[lo:hi], order[lo:hi])]
            yield self._batch((img, mask, dist, lu, stats))
        flag = int(self._err.item())     # the one read of the epoch
        if flag:
            self._err.zero_()
            raise RuntimeError(f"pool gather: error flag {flag} (1: sample index outside its pool, 2: odd turn of a "
                               "non-square tile, 4: source outside the pool list); those samples were zero-filled")


class PoolLoader(_GatherLoader):
    """Batches of one ``DevicePool`` in the reference's format: ``{"main": (img f32 [B,C,H,W], mask i64 [B,H,W], distmap,
    lu i64 [B,H,W], stats)}`` (``wrap=False``: the bare tuple of ``test_dataloader``), after one ``epoch_plan`` per epoch
    (three small uploads: idx, geo, bc; one pool needs no src).  ``len()`` is ``len(pool) // batch_size``: a pool smaller
    than one batch yields nothing.  Everything else is ``_GatherLoader``'s."""

    def __init__(self, pool: DevicePool, batch_size: int, train: bool = False, in_channels: int = 3, classes: int = 2,
                 seed: int = 0, wrap: bool = True, distmap: bool = True, trainer=None, mean=MEAN, std=STD):
        self.pool, self.wrap = pool, bool(wrap)
        super().__init__([pool], [batch_size], train, in_channels, classes, seed, distmap, trainer, mean, std)

    def plan(self, epoch: int):
        """the host plan of ``epoch`` (what ``__iter__`` uploads)"""
        p = self.pool
        return epoch_plan(len(p), self.batch_size, epoch, self.seed, self.train, p.height == p.width)

    def __len__(self):
        return len(self.pool) // self.batch_size

    def _host_plan(self, epoch: int):
        return (None,) + self.plan(epoch)

    def _batch(self, item):
        return {"main": item} if self.wrap else item


class CombinedPoolLoader(_GatherLoader):
    """Several pools (the main set and the extra sets of ``pattern_extra``): every batch is a ``CombinedBatch`` of
    ``batch_sizes[0]`` main samples followed by ``batch_sizes[j]`` samples of every extra pool, rows of the epoch's
    ``combined_plan`` (four small uploads per epoch: src, idx, geo, bc; three with one pool).  ``len()`` is the longest
    source's batch count; shorter ones cycle, and a pool smaller than its batch size is a ``ValueError``.  Everything
    else is ``_GatherLoader``'s."""

    def plan(self, epoch: int):
        """the host plan of ``epoch``: ``combined_plan`` of the pools' sizes"""
        p = self.pools[0]
        return combined_plan([len(q) for q in self.pools], self.batch_sizes, epoch, self.seed, self.train,
                             p.height == p.width)

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._len = self.plan(0)[0]          # (raises for a pool too small for one batch)

    def __len__(self):
        return self._len

    def _host_plan(self, epoch: int):
        _, src, *rows = self.plan(epoch)
        return (src if len(self.pools) > 1 else None, *rows)

    def _batch(self, item):
        return CombinedBatch(item, self.batch_sizes)
