"""``DeadtreesDataModule`` surface (reference deadtrees/data/deadtreedata.py:192-405) with two sources.

The reference streams webdataset shards through albumentations on CPU workers; neither package is available here
(SURVEY §8c), and at >400 tiles/s/GPU that loader is the limiter anyway (§8 f2).  This module keeps the constructor /
``setup`` / ``*_dataloader`` surface and the batch formats (``{"main": (img, mask, distmap, lu, stats)}`` for train/val
:348-395, a bare tuple for test :397-405).  Without shards it fills them with synthetic tiles of the reference's shape;
with ``*.tar`` shards it reads them once (``shards.py``, stdlib ``tarfile`` + PIL) into device-resident pools and one HIP
kernel makes every batch (``pool.py``).  ``val_transform`` is the reference normalisation (:148-154) in numpy.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .distmap import distmaps_for_batch, distmaps_on_device
from .synthetic import MEAN, STD, synth_batch


class DeadtreeDatasetConfig:
    """reference deadtreedata.py:27-34"""
    mean = np.array(MEAN)
    std = np.array(STD)
    tile_size = 256
    fractions = [0.7, 0.2, 0.1]


def val_transform(image: np.ndarray, mask: Optional[np.ndarray] = None):
    """albumentations ``Normalize(mean, std)`` + ``ToTensorV2`` of deadtreedata.py:148-154: HWC uint8 -> CHW f32"""
    c = image.shape[-1]
    mean = (np.asarray(MEAN[:c], dtype=np.float32) * 255.0)
    inv = 1.0 / (np.asarray(STD[:c], dtype=np.float32) * 255.0)
    img = (image.astype(np.float32) - mean) * inv
    out = {"image": torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1)))}
    if mask is not None:
        out["mask"] = torch.from_numpy(mask)
    return out


def draw_train_params(batch: int, rng: np.random.Generator):
    """Per-sample random parameters of the reference's ``train_transform`` (deadtreedata.py:128-146):
    OneOf([HorizontalFlip, VerticalFlip], p=0.5) -> 25 % each; RandomRotate90(p=0.5) -> k = randint(0, 3);
    RandomBrightnessContrast(p=0.5, brightness_limit=0.2, contrast_limit=0.15): alpha = 1 + U(-.15, .15),
    beta = U(-.2, .2).  Returns (geo int32 [B,2], bc float32 [B,2]) for ``train_transform_device``."""
    geo = np.zeros((batch, 2), np.int32)
    bc = np.tile(np.array([1.0, 0.0], np.float32), (batch, 1))
    for b in range(batch):
        if rng.random() < 0.5:
            geo[b, 0] = 1 if rng.random() < 0.5 else 2
        if rng.random() < 0.5:
            geo[b, 1] = int(rng.integers(0, 4))
        if rng.random() < 0.5:
            bc[b] = (1.0 + rng.uniform(-0.15, 0.15), rng.uniform(-0.2, 0.2))
    return torch.from_numpy(geo), torch.from_numpy(bc)


def train_transform_device(tiles_u8_nhwc: torch.Tensor, mask: torch.Tensor, lu: Optional[torch.Tensor],
                           rng: np.random.Generator, in_channels: int = 3):
    """``train_transform`` + ``transform`` (deadtreedata.py:128-146,165-176) for a whole batch already in HBM:
    uint8 [B,H,W,4] tiles, int64 masks (and land-use maps) -> (NCHW fp32 image batch, mask, lu) with ONE fused
    flip/rot90/brightness-contrast/normalise pass and one gather per label map (kernels `dt_augment_*`)."""
    from .. import ops
    B = tiles_u8_nhwc.shape[0]
    geo, bc = draw_train_params(B, rng)
    geo, bc = geo.to(tiles_u8_nhwc.device), bc.to(tiles_u8_nhwc.device)
    img = ops.augment_normalize_u8(tiles_u8_nhwc, geo, bc, MEAN, STD, in_channels).permute(0, 3, 1, 2)
    mask = ops.augment_labels(mask.long(), geo)
    lu = ops.augment_labels(lu.long(), geo) if lu is not None else None
    return img, mask, lu


_TRAIN_RNG = np.random.default_rng()


def train_transform(image: np.ndarray, mask: Optional[np.ndarray] = None, masks=None):
    """The reference's module-level ``train_transform`` (deadtreedata.py:128-146, an albumentations ``Compose``) as a
    callable on ONE sample: HWC uint8 ``image`` (+ ``mask`` or a list ``masks``, as the reference's ``transform`` passes
    them, :165-176) -> ``{"image": CHW f32 tensor, "mask": ..., "masks": [...]}`` with the same random flip / rot90 /
    brightness-contrast draw for image and label maps.  Runs ``train_transform_device`` on a batch of one — the HIP
    augmentation kernels; there is no CPU path (raises without a HIP device)."""
    if not torch.cuda.is_available():
        raise RuntimeError("deadtrees_amd train_transform runs the HIP augmentation kernels: no HIP device, no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device())
    c = image.shape[-1]
    maps = ([] if mask is None else [mask]) + list(masks or [])
    tiles = torch.from_numpy(np.ascontiguousarray(image))[None].to(dev)
    geo, bc = draw_train_params(1, _TRAIN_RNG)
    geo, bc = geo.to(dev), bc.to(dev)
    from .. import ops
    img = ops.augment_normalize_u8(tiles, geo, bc, MEAN, STD, c).permute(0, 3, 1, 2)[0].contiguous()
    outs = [ops.augment_labels(torch.from_numpy(np.ascontiguousarray(m))[None].to(dev).long(), geo)[0].to(
        torch.from_numpy(np.asarray(m)).dtype) for m in maps]
    out = {"image": img}
    if mask is not None:
        out["mask"] = outs[0]
    if masks is not None:
        out["masks"] = outs[(0 if mask is None else 1):]
    return out


class _SyntheticLoader:
    def __init__(self, n_batches, batch_size, size, in_channels, classes, seed, wrap_main, device, with_distmap):
        self.n, self.bs, self.size, self.c, self.k = n_batches, batch_size, size, in_channels, classes
        self.seed, self.wrap, self.device, self.with_distmap = seed, wrap_main, device, with_distmap

    def __len__(self):
        return self.n

    def __iter__(self):
        for i in range(self.n):
            img, mask = synth_batch(self.bs, self.size, self.size, self.c, self.k, seed=self.seed + i)
            on_gpu = bool(self.device) and str(self.device).startswith("cuda")
            # labels headed for HBM get their maps from the device EDT kernel below; a host-only loader attaches
            # them the way the reference's loader does (scipy, data/deadtreedata.py:182-185)
            dist = None if (on_gpu or not self.with_distmap) else distmaps_for_batch(mask, self.k)
            lu = torch.ones_like(mask)
            stats = [{"file": f"synthetic_{self.seed + i}_{j}", "frac": float((mask[j] > 0).float().mean())}
                     for j in range(self.bs)]
            if self.device:
                img, mask, lu = (t.to(self.device) for t in (img, mask, lu))
                if self.with_distmap:
                    dist = distmaps_on_device(mask, self.k) if on_gpu else dist.to(self.device)
            item = (img, mask, dist, lu, stats)
            yield {"main": item} if self.wrap else item


class DeadtreesDataModule:
    """Two sources behind the reference's surface.  Without shards: synthetic tiles (``_SyntheticLoader``).  With
    ``*.tar`` shards in ``data_dir`` (one directory + ``pattern``, split by ``split_shards``; or a list of three
    directories, the reference's train / val / test layout): ``setup`` decodes every shard once into device-resident
    pools (``data/pool.py``) and the ``*_dataloader()`` methods return ``PoolLoader``s, whose batches one HIP gather
    kernel makes.  ``rank`` / ``world``: under data parallelism every rank reads ``shards_for_rank`` of the train shards;
    ``seed`` seeds the epoch plans; ``max_resident_bytes`` bounds each pool (default: half of the free device memory).

    ``pattern_extra`` / ``batch_size_extra`` (reference :218-238, 318-395; its ``deadtrees_multi_datasets*`` configs): further
    shard sets of the one directory.  Each is split train / val in the main set's proportion into pools of its own
    (``extra_pools``); the train and val loaders then are ``CombinedPoolLoader``s whose batches hold ``batch_size -
    sum(batch_size_extra)`` main samples under ``"main"`` and ``batch_size_extra[i]`` samples of set i under ``"extra_i"``,
    the shorter sets cycling, all from one kernel launch.  The test loader stays the main set alone.

    ``rasters`` (instead of ``data_dir``): the ortho rasters themselves, a sequence or re-iterable of ``(key, rgbn, mask |
    None, lu | None)`` items as ``DevicePool.from_rasters`` takes them (``data/rasters.py``).  ``setup`` sorts the raster
    keys and splits them with ``split_shards`` — by raster, never by sub-tile, so neighbouring sub-tiles do not straddle
    train and val — takes ``shards_for_rank`` of the train part and fills the three pools with ``from_rasters``.
    ``raster_conf``: ``tile_size`` (default: this module's), ``source_dim`` (2048), ``select`` ("dead"), and for the
    random set ``oversample`` (2) and ``seed`` (42).  ``batch_size_extra=[k]`` adds the random set of
    ``raster_training_sets`` (zero masks) as the one extra pool of the train and val loaders.  ``mean`` / ``std`` (default:
    the reference's constants) go to the loaders; ``normalise="rasters"`` computes them with ``band_stats`` over the train
    part (``raster_conf["reference_denominator"]``, default True)."""

    def __init__(self, data_dir=None, pattern=None, pattern_extra=None, batch_size_extra=None,
                 train_dataloader_conf=None, val_dataloader_conf=None, test_dataloader_conf=None,
                 synthetic_batches: int = 8, tile_size: int = 256, device: Optional[str] = None,
                 rank: int = 0, world: int = 1, seed: int = 0, max_resident_bytes: Optional[int] = None,
                 rasters=None, raster_conf=None, mean=None, std=None, normalise: Optional[str] = None):
        self.data_dir, self.pattern = data_dir, pattern
        self.rasters, self.raster_conf = rasters, dict(raster_conf or {})
        self.mean = tuple(MEAN if mean is None else mean)
        self.std = tuple(STD if std is None else std)
        self.normalise = normalise
        if normalise not in (None, "rasters"):
            raise ValueError(f"normalise {normalise!r}: None (the mean / std given) or 'rasters'")
        if rasters is None and (normalise or raster_conf):
            raise ValueError("normalise='rasters' and raster_conf need rasters=")
        if rasters is not None:
            if data_dir or pattern or pattern_extra:
                raise ValueError("rasters= is an alternative to data_dir / pattern / pattern_extra: give one source")
            if batch_size_extra and len(batch_size_extra) > 1:
                raise ValueError(f"rasters= has one extra set, the random sub-tiles: batch_size_extra {list(batch_size_extra)} "
                                 "has more than one entry")
            if iter(rasters) is rasters:
                raise ValueError("rasters= is read more than once: pass a sequence or a re-iterable, not an iterator")
        self.train_conf = dict(train_dataloader_conf or {})
        self.val_conf = dict(val_dataloader_conf or {})
        self.test_conf = dict(test_dataloader_conf or {})
        self.synthetic_batches, self.tile_size, self.device = synthetic_batches, tile_size, device
        self.in_channels, self.classes = 3, 2
        self.rank, self.world, self.seed, self.max_resident_bytes = rank, world, seed, max_resident_bytes
        self.pools = None
        self.extra_pools = []
        self.layout, self.data_shards = _find_shards(data_dir, pattern)
        self.pattern_extra = [str(p) for p in (pattern_extra or [])]
        self.batch_size_extra = [int(b) for b in (batch_size_extra or [])]
        self.data_shards_extra = []
        if rasters is not None:
            self.layout, self.data_shards = "rasters", []
            if self.batch_size_extra and min(self.batch_size_extra) < 1:
                raise ValueError(f"batch_size_extra {self.batch_size_extra}: every extra set gives at least one sample")
        elif self.pattern_extra or self.batch_size_extra:
            if isinstance(data_dir, (list, tuple)):
                raise ValueError("Combining pattern_extra with train/val/test layout not allowed")
            if not self.batch_size_extra:
                raise ValueError("<pattern_extra> provided but no <batch_size_extra> ratio found")
            if not self.pattern_extra:
                raise ValueError("<batch_size_extra> provided but no <pattern_extra> found")
            if len(self.batch_size_extra) != len(self.pattern_extra):
                raise ValueError("Len of <pattern_extra> and <batch_size_extra> don't match")
            if min(self.batch_size_extra) < 1:
                raise ValueError(f"batch_size_extra {self.batch_size_extra}: every extra set gives at least one sample")
            if self.data_shards is None:
                raise NotImplementedError("pattern_extra / batch_size_extra with the synthetic source (no shard matches "
                                          "`pattern` in data_dir) are not built: extra sets are shard sets")
            from pathlib import Path
            for p in self.pattern_extra:
                shards = sorted(str(q) for q in Path(str(data_dir)).glob(p))
                if not shards:
                    raise NotImplementedError(f"pattern_extra {p!r} matches no shard in {data_dir}: an extra set without "
                                              "samples cannot be cycled")
                self.data_shards_extra.append(shards)

    def setup(self, stage=None, split_fractions=None, in_channels: int = 3, classes: int = 2):
        self.in_channels, self.classes = in_channels, classes
        if self.data_shards is None:
            return
        if self.rasters is not None:
            return self._setup_rasters(split_fractions)
        from .pool import DevicePool
        from .shards import shards_for_rank, split_shards
        if self.layout == "single_directory":
            fractions = DeadtreeDatasetConfig.fractions if split_fractions is None else split_fractions
            train, valid, test = split_shards(self.data_shards, fractions)
        else:
            train, valid, test = ([str(s) for s in part] for part in self.data_shards)
        self.shard_split = {"train": shards_for_rank(train, self.rank, self.world), "val": valid, "test": test or None}
        self.pools = {name: DevicePool(shards, device=self.device, max_resident_bytes=self.max_resident_bytes)
                      for name, shards in self.shard_split.items() if shards}
        # every extra set is split train / val in the proportion of the main split (reference :318-346)
        self.extra_pools, self.extra_shard_split = [], []
        train_frac = len(train) / (len(train) + len(valid))
        main = self.pools["train"]
        for pattern, shards in zip(self.pattern_extra, self.data_shards_extra):
            if len(shards) < 2:
                raise ValueError(f"pattern_extra {pattern!r} matches {len(shards)} shard: a train and a val part need "
                                 "one shard each")
            e_train, e_valid, _ = split_shards(shards, [train_frac, 1 - train_frac])
            if not e_train or not e_valid:
                raise ValueError(f"pattern_extra {pattern!r}: the split of its {len(shards)} shards leaves the "
                                 f"{'train' if not e_train else 'val'} part empty")
            split = {"train": shards_for_rank(e_train, self.rank, self.world), "val": e_valid}
            pools = {name: DevicePool(part, device=self.device, max_resident_bytes=self.max_resident_bytes)
                     for name, part in split.items()}
            for name, pool in pools.items():
                if (pool.height, pool.width) != (main.height, main.width):
                    raise ValueError(f"pattern_extra {pattern!r}: {name} tiles are {pool.height}x{pool.width}, those of "
                                     f"the main set {main.height}x{main.width}")
            self.extra_shard_split.append(split)
            self.extra_pools.append(pools)

    def _raster_part(self, keys):
        """the items of the rasters ``keys``, in that order when ``rasters`` can be indexed, else in its own order"""
        if hasattr(self.rasters, "__getitem__"):
            at = {str(item[0]): i for i, item in enumerate(self.rasters)}
            return [self.rasters[at[k]] for k in keys]
        wanted, src = set(keys), self.rasters

        class Part:
            def __iter__(self):
                return (item for item in src if str(item[0]) in wanted)
        return Part()

    def _setup_rasters(self, split_fractions):
        from .rasters import OVERSAMPLE_FACTOR, band_stats, pool_from_rasters, raster_training_sets
        from .shards import shards_for_rank, split_shards
        keys = sorted(str(item[0]) for item in self.rasters)
        if len(set(keys)) != len(keys):
            raise ValueError("rasters=: the raster keys are not unique")
        fractions = DeadtreeDatasetConfig.fractions if split_fractions is None else split_fractions
        train, valid, test = split_shards(keys, fractions)
        self.shard_split = {"train": shards_for_rank(train, self.rank, self.world), "val": valid, "test": test or None}
        conf = self.raster_conf
        select = conf.get("select", "dead")
        kw = dict(tile_size=int(conf.get("tile_size", self.tile_size)), source_dim=int(conf.get("source_dim", 2048)),
                  device=self.device, max_resident_bytes=self.max_resident_bytes)
        if self.batch_size_extra and select != "dead":
            raise ValueError("batch_size_extra with rasters= adds the random set, which is drawn beside the 'dead' set: "
                             f"select is {select!r}")
        self.pools, extra, censuses = {}, {}, None
        for name, part in self.shard_split.items():
            if not part:
                continue
            items = self._raster_part(part)
            if self.batch_size_extra and name != "test":
                sets = raster_training_sets(items, oversample=int(conf.get("oversample", OVERSAMPLE_FACTOR)),
                                            seed=int(conf.get("seed", 42)), **kw)
                self.pools[name], extra[name], record = sets["dead"], sets["random"], sets
            else:
                record = {}
                self.pools[name] = pool_from_rasters(items, select=select, masks="keep", record=record, **kw)
            if name == "train":
                censuses = record["censuses"]
        self.extra_pools, self.extra_shard_split = ([extra], [dict(self.shard_split)]) if self.batch_size_extra else ([], [])
        if self.normalise == "rasters":
            stats = band_stats(censuses, kw["source_dim"], kw["tile_size"],
                               reference_denominator=bool(conf.get("reference_denominator", True)))
            self.mean, self.std, self.band_stats = tuple(stats["mean"]), tuple(stats["std"]), stats

    def _loader(self, conf, seed, wrap):
        return _SyntheticLoader(self.synthetic_batches, int(conf.get("batch_size", 8)), self.tile_size,
                                self.in_channels, self.classes, seed, wrap, self.device, True)

    def _need_setup(self):
        if self.pools is None:
            raise RuntimeError("DeadtreesDataModule: call setup() before asking for a loader")

    def _device_pools(self, name, extra=False):
        """the ``name`` pool, followed by those of the extra sets if asked: after setup(), in the split, on the device"""
        self._need_setup()
        if name not in self.pools:
            raise RuntimeError(f"DeadtreesDataModule: the split has no {name} shards")
        pools = [self.pools[name]] + ([e[name] for e in self.extra_pools] if extra else [])
        if not all(p.on_device for p in pools):
            raise RuntimeError("deadtrees_amd loaders run the HIP gather kernel on a device-resident pool: no HIP device, "
                               "no CPU fallback")
        return pools

    def _pool_loader(self, name, conf, train, wrap, trainer=None, distmap=True):
        from .pool import PoolLoader
        return PoolLoader(self._device_pools(name)[0], int(conf.get("batch_size", 8)), train=train,
                          in_channels=self.in_channels, classes=self.classes, seed=self.seed, wrap=wrap, distmap=distmap,
                          trainer=trainer, mean=self.mean, std=self.std)

    def _combined_loader(self, name, conf, train, trainer=None, distmap=True):
        from .pool import CombinedPoolLoader
        self._need_setup()
        batch_size = int(conf.get("batch_size", 8))
        main = batch_size - sum(self.batch_size_extra)
        if main < 1:
            raise ValueError(f"{name} batch_size {batch_size} leaves {main} main samples beside batch_size_extra "
                             f"{self.batch_size_extra}")
        return CombinedPoolLoader(self._device_pools(name, extra=True), [main] + self.batch_size_extra, train=train,
                                  in_channels=self.in_channels, classes=self.classes, seed=self.seed, distmap=distmap,
                                  trainer=trainer, mean=self.mean, std=self.std)

    def train_dataloader(self, trainer=None, distmap: Optional[bool] = None):
        """trainer: a ``HipTrainer(graph=True)`` whose captured step the loader feeds in place (``PoolLoader``); its
        batches then carry no distance maps unless ``distmap=True`` — the trainer computes them inside the captured step
        when a boundary loss needs them."""
        if self.data_shards is None:
            return self._loader(self.train_conf, 1000, True)
        distmap = (trainer is None) if distmap is None else distmap
        if self.batch_size_extra:
            return self._combined_loader("train", self.train_conf, True, trainer, distmap)
        return self._pool_loader("train", self.train_conf, True, True, trainer, distmap)

    def val_dataloader(self):
        if self.data_shards is None:
            return self._loader(self.val_conf, 2000, True)
        if self.batch_size_extra:
            return self._combined_loader("val", self.val_conf, False)
        return self._pool_loader("val", self.val_conf, False, True)

    def test_dataloader(self):
        if self.data_shards is None:
            return self._loader(self.test_conf, 3000, False)
        return self._pool_loader("test", self.test_conf, False, False)


def _find_shards(data_dir, pattern):
    """(layout, shards): ("single_directory", sorted paths) for one directory, ("train/val/test", three sorted lists) for
    a list of three (reference deadtreedata.py:207-212); (None, None) when there is no shard (the synthetic source)"""
    from pathlib import Path
    if not data_dir:
        return None, None
    pattern = pattern or "*.tar"
    if isinstance(data_dir, (list, tuple)):
        if len(data_dir) != 3:
            raise ValueError("data_dir as a list is the train / val / test layout: three directories")
        parts = [sorted(str(p) for p in Path(d).glob(pattern)) for d in data_dir]
        if not any(parts):
            return None, None
        if not (parts[0] and parts[1]):
            raise ValueError(f"train / val / test layout: no shards matching {pattern!r} in the train or val directory")
        return "train/val/test", parts
    shards = sorted(str(p) for p in Path(str(data_dir)).glob(pattern))
    return ("single_directory", shards) if shards else (None, None)


def data_dir_has_shards(data_dir) -> bool:
    import glob
    import os
    return bool(data_dir) and bool(glob.glob(os.path.join(str(data_dir), "*.tar")))
