"""Training samples and normalisation constants straight from ortho rasters.

The reference prepares training data off line: ``scripts/createdataset.py`` cuts every 2048 x 2048 ortho (rgbn), its
dead-tree mask and its forest (land-use) mask into 256 x 256 sub-tiles, drops the blank ones, writes those with dead
pixels into ``*.tar`` shards together with a random draw of the others, and ``scripts/computestats.py`` derives the band
means / standard deviations from the same rasters.  Both need rioxarray / webdataset / GDAL.  Everything the shards carry
is a function of the raster bytes, so here it is computed from the rasters themselves, on the device when there is one
(csrc/raster_cut.hip: one pass gives the census of every sub-tile and writes the selected ones into a ``DevicePool``), and
this module states the contract in numpy (``cut_raster_host``: the yardstick of the GPU tests and the path taken without a
HIP device).

Contract (createdataset.py:53-194, 378-425; computestats.py:111-161):
  cut     rgbn uint8 [4,h,w] with h, w <= S stands in the top-left corner of a zero [4,S,S] array; mask [h,w] likewise
          (None: zeros); lu [h,w] likewise (None: ones everywhere, the padding included); ``make_blocks_vectorized(x, t)``
          gives the n = (S / t)^2 sub-tiles; sub-tile i of raster ``stem`` is called ``f"{stem}_{i:03}"``.
  blank   a sub-tile with min == max over its four bands gives no sample and no row.
  frac    ``round(count_nonzero(mask_i) / t^2 * 100, 2)`` (a percentage); status 1 iff frac > 0.  The rounding is part of
          the contract: at t = 256 three dead pixels are 0.0 (status 0), four are 0.01 (status 1).
  random  ``oversample * n_dead`` names drawn from all sub-tile names minus the dead ones, cut with a zero mask and the
          raster's lu; drawn names that are blank are dropped.
  stats   rasters that are not S x S or whose bytes are all in {0, 255} are skipped; of the rest the sub-tiles with min !=
          max in band 0 count: mean_c = sum_tiles(sum x / t^2) / (cnt + 1), std_c = sqrt(sum_tiles(sum (x - mean_c)^2 /
          t^2) / (cnt + 1)) with x = byte / 255.

Two deliberate differences: the random draw is ``np.random.default_rng(seed).choice(sorted(names), size,
replace=False)`` (the reference samples a ``set``, whose order changes from process to process), and the ``cnt + 1``
denominator of the statistics can be switched to ``cnt`` (``reference_denominator=False``).
"""
from __future__ import annotations

import csv
import datetime
import json
from typing import Callable, Iterable, Optional, Sequence, Union

import numpy as np
import torch

from .._lib import (CENSUS_B0MAX, CENSUS_B0MIN, CENSUS_COLS, CENSUS_DEAD, CENSUS_MID, CENSUS_SUM, CENSUS_SUMSQ, CENSUS_VMAX,
                    CENSUS_VMIN)
from ..deployment.tiler import make_blocks_vectorized

OVERSAMPLE_FACTOR = 2       # createdataset.py:47
BANDS = ("red", "green", "blue", "nir")


# ---------------------------------------------------------------------------------------------- the contract in numpy
def _check_geometry(S: int, t: int, h: int, w: int) -> int:
    if t < 32 or t % 32:
        raise ValueError(f"tile size {t} must be a positive multiple of 32 (the network's five stride-2 stages)")
    if S < t or S % t:
        raise ValueError(f"source_dim {S} must be a multiple of the tile size {t}")
    if not (1 <= h <= S and 1 <= w <= S):
        raise ValueError(f"raster {h}x{w} must be 1..{S} in height and width")
    return (S // t) ** 2


def _padded(x: Optional[np.ndarray], bands: int, h: int, w: int, S: int, none_fill: int) -> np.ndarray:
    if x is None:
        return np.full((bands, S, S), none_fill, np.uint8)
    x = np.asarray(x)
    if x.dtype != np.uint8 or x.shape[-2:] != (h, w):
        raise ValueError(f"raster maps must be uint8 [{h},{w}], not {x.dtype} {x.shape}")
    out = np.zeros((bands, S, S), np.uint8)
    out[:, :h, :w] = x.reshape(bands, h, w)
    return out


def cut_raster_host(rgbn: np.ndarray, mask: Optional[np.ndarray], lu: Optional[np.ndarray], S: int, t: int):
    """The cut and the census of one raster: ``(images uint8 [n,t,t,4], masks uint8 [n,t,t], lu uint8 [n,t,t], sums uint64
    [n], census int64 [n,16])`` for ALL n sub-tiles, blank ones included (the census tells them apart).  Census columns
    (``_lib.CENSUS_*``, over the padded sub-tile): dead = non-zero mask pixels; vmin / vmax over the four bands; b0min /
    b0max of band 0; mid = image bytes not in {0, 255}; sum[4] / sumsq[4] per band; zeros up to 16."""
    rgbn = np.asarray(rgbn)
    if rgbn.dtype != np.uint8 or rgbn.ndim != 3 or rgbn.shape[0] != 4:
        raise ValueError(f"rgbn must be uint8 [4,h,w], not {rgbn.dtype} {rgbn.shape}")
    h, w = rgbn.shape[1:]
    n = _check_geometry(int(S), int(t), h, w)
    img = make_blocks_vectorized(_padded(rgbn, 4, h, w, S, 0), t)                  # [n,4,t,t]
    msk = make_blocks_vectorized(_padded(mask, 1, h, w, S, 0), t)[:, 0]
    lnd = make_blocks_vectorized(_padded(lu, 1, h, w, S, 1), t)[:, 0]
    flat = img.reshape(n, 4, t * t)
    wide = flat.astype(np.int64)
    census = np.zeros((n, CENSUS_COLS), np.int64)
    census[:, CENSUS_DEAD] = np.count_nonzero(msk.reshape(n, -1), axis=1)
    census[:, CENSUS_VMIN] = flat.min(axis=(1, 2))
    census[:, CENSUS_VMAX] = flat.max(axis=(1, 2))
    census[:, CENSUS_B0MIN] = flat[:, 0].min(axis=1)
    census[:, CENSUS_B0MAX] = flat[:, 0].max(axis=1)
    census[:, CENSUS_MID] = np.count_nonzero((flat != 0) & (flat != 255), axis=(1, 2))
    census[:, CENSUS_SUM:CENSUS_SUM + 4] = wide.sum(axis=2)
    census[:, CENSUS_SUMSQ:CENSUS_SUMSQ + 4] = (wide * wide).sum(axis=2)
    images = np.ascontiguousarray(img.transpose(0, 2, 3, 1))
    sums = census[:, CENSUS_SUM:CENSUS_SUM + 4].sum(axis=1).astype(np.uint64)
    return images, np.ascontiguousarray(msk), np.ascontiguousarray(lnd), sums, census


def subtile_names(key: str, n: int) -> list:
    return [f"{key}_{i:03}" for i in range(n)]


def _census_array(census) -> np.ndarray:
    census = census.cpu().numpy() if isinstance(census, torch.Tensor) else np.asarray(census)
    if census.ndim != 2 or census.shape[1] != CENSUS_COLS:
        raise ValueError(f"a census is int64 [n,{CENSUS_COLS}], not {census.shape}")
    return census.astype(np.int64, copy=False)


def nonblank(census) -> np.ndarray:
    """bool [n]: the sub-tiles that give a sample (min != max over the four bands)"""
    census = _census_array(census)
    return census[:, CENSUS_VMIN] != census[:, CENSUS_VMAX]


def fracs(census, t: int) -> list:
    """the reference's dead-pixel percentage of every sub-tile, rounded as it rounds it (a Python float each)"""
    return [round(float(d) / (t * t) * 100, 2) for d in _census_array(census)[:, CENSUS_DEAD].tolist()]


def subtile_table(key: str, census, t: int) -> list:
    """rows ``(name, frac, status)`` of the non-blank sub-tiles of raster ``key`` in sub-tile order: what
    createdataset.py writes into its ``tile,frac,status`` file (there as strings)"""
    keep = nonblank(census)
    return [(name, frac, 1 if frac > 0 else 0)
            for name, frac, ok in zip(subtile_names(key, len(keep)), fracs(census, t), keep.tolist()) if ok]


def write_subtile_csv(rows: Iterable, path) -> None:
    """the reference's stats file: header ``tile,frac,status``, one row per non-blank sub-tile"""
    with open(str(path), "w", newline="") as f:
        out = csv.writer(f, lineterminator="\n")
        out.writerow(["tile", "frac", "status"])
        for name, frac, status in rows:
            out.writerow([name, str(frac), str(status)])


# ---------------------------------------------------------------------------------------------- items
def _open(x, mode: str) -> np.ndarray:
    """an array as it is; anything else is a path (or file object) that PIL opens, converted as ``shards._decode`` does"""
    if isinstance(x, np.ndarray):
        return x
    if isinstance(x, torch.Tensor):
        return x.cpu().numpy()
    from PIL import Image
    with Image.open(x) as img:
        img.load()
        arr = np.asarray(img.convert(mode))
    return np.ascontiguousarray(arr.transpose(2, 0, 1)) if mode == "RGBA" else arr


def load_item(item, keep_polygons: bool = False):
    """``(key, rgbn, mask | None, lu | None)`` with arrays or paths -> the same with uint8 arrays [4,h,w] / [h,w].  A mask
    or lu given as a ``PolygonSet`` in the raster's pixel coordinates (``data/polygons.py``) is burnt by ``rasterize_host``,
    or, with ``keep_polygons``, handed on as it is for the caller to burn on the device."""
    from .polygons import PolygonSet, rasterize_host
    if len(item) != 4:
        raise ValueError(f"a raster item is (key, rgbn, mask | None, lu | None), not {len(item)} fields")
    key, rgbn, mask, lu = item
    rgbn = _open(rgbn, "RGBA")
    if rgbn.dtype != np.uint8 or rgbn.ndim != 3 or rgbn.shape[0] != 4:
        raise ValueError(f"raster {key!r}: rgbn must be uint8 [4,h,w], not {rgbn.dtype} {rgbn.shape}")
    maps = []
    for name, m in (("mask", mask), ("lu", lu)):
        if isinstance(m, PolygonSet):
            maps.append(m if keep_polygons else rasterize_host(m, rgbn.shape[1], rgbn.shape[2]))
            continue
        m = None if m is None else _open(m, "L")
        if m is not None and (m.dtype != np.uint8 or m.shape != rgbn.shape[1:]):
            raise ValueError(f"raster {key!r}: {name} must be uint8 {list(rgbn.shape[1:])}, not {m.dtype} {list(m.shape)}")
        maps.append(m)
    return str(key), rgbn, maps[0], maps[1]


def _selection(select, names, census, t) -> np.ndarray:
    keep = nonblank(census)
    if callable(select):
        chosen = np.asarray(select(names, census), dtype=bool)
        if chosen.shape != keep.shape:
            raise ValueError(f"select returned shape {chosen.shape} for {len(names)} sub-tiles")
        return keep & chosen
    if select == "valid":
        return keep
    if select == "dead":
        return keep & np.array([f > 0 for f in fracs(census, t)], dtype=bool)
    raise ValueError(f"select {select!r}: 'dead', 'valid' or a callable (names, census) -> bool[n]")


class _DeviceRows:
    """the four pool tensors with spare rows: ``reserve`` doubles them (copying what is filled) up to the bound"""

    def __init__(self, t, dev, max_bytes):
        self.t, self.dev, self.max_bytes, self.cap, self.at = t, dev, max_bytes, 0, 0
        self.tensors = self._alloc(0)

    def _alloc(self, rows):
        t, dev = self.t, self.dev
        return (torch.empty((rows, t, t, 4), dtype=torch.uint8, device=dev),
                torch.empty((rows, t, t), dtype=torch.uint8, device=dev),
                torch.empty((rows, t, t), dtype=torch.uint8, device=dev), torch.empty(rows, dtype=torch.int64, device=dev))

    def row_bytes(self):
        return self.t * self.t * 6 + 8

    def check(self, rows):
        need = rows * self.row_bytes()
        if self.max_bytes is not None and need > self.max_bytes:
            raise ValueError(f"DevicePool: {rows} samples of {self.t}x{self.t} need {need} bytes resident, "
                             f"max_resident_bytes is {int(self.max_bytes)} (streaming a split that does not fit is not "
                             "supported)")

    def reserve(self, rows):
        if rows <= self.cap:
            return
        self.check(rows)
        cap = max(rows, 2 * self.cap)
        if self.max_bytes is not None:
            cap = max(rows, min(cap, int(self.max_bytes) // self.row_bytes()))
        self._move(cap)

    def _move(self, cap):
        new = self._alloc(cap)
        for a, b in zip(new, self.tensors):
            a[:self.at].copy_(b[:self.at])
        self.tensors, self.cap = new, cap

    def finish(self):
        if self.cap != self.at:
            self._move(self.at)
        return self.tensors


def pool_from_rasters(items, tile_size: int = 256, source_dim: int = 2048, select: Union[str, Callable] = "dead",
                      masks: str = "keep", device=None, max_resident_bytes: Optional[int] = None, record: Optional[dict] = None):
    """What ``DevicePool.from_rasters`` does (see there).  ``record``: a dict that receives ``keys`` (the raster keys in
    order), ``table`` (the ``subtile_table`` rows of all rasters) and ``censuses`` (``(census, (h, w))`` per raster, as
    ``band_stats`` takes them)."""
    from .polygons import PolygonSet, rasterize
    from .pool import DevicePool, _device_or_none
    t, S = int(tile_size), int(source_dim)
    if masks not in ("keep", "zero"):
        raise ValueError(f"masks {masks!r}: 'keep' or 'zero'")
    dev = _device_or_none(device)
    on_gpu = dev is not None and dev.type == "cuda"
    if max_resident_bytes is None and on_gpu:
        max_resident_bytes = torch.cuda.mem_get_info(dev)[0] // 2
    _check_geometry(S, t, 1, 1)
    n = (S // t) ** 2
    keys, table, censuses, stats = [], [], [], []
    if on_gpu:
        from .. import ops
        rows = _DeviceRows(t, dev, max_resident_bytes)
        pinned = torch.empty(6 * S * S, dtype=torch.uint8, pin_memory=True)       # one raster with both maps
        staged = torch.empty(6 * S * S, dtype=torch.uint8, device=dev)
        census_dev = torch.empty((n, CENSUS_COLS), dtype=torch.int64, device=dev)
    else:
        parts, count = [], 0
    for item in items:
        key, rgbn, mask, lu = load_item(item, keep_polygons=on_gpu)
        h, w = rgbn.shape[1:]
        _check_geometry(S, t, h, w)
        names = subtile_names(key, n)
        if on_gpu:
            hw, at = h * w, 4 * h * w
            host = pinned.numpy()
            host[:at] = rgbn.reshape(-1)
            views = [None, None]
            for j, m in enumerate((mask, lu)):
                if m is not None and not isinstance(m, PolygonSet):
                    host[at:at + hw] = m.reshape(-1)
                    views[j] = (at, at + hw)
                    at += hw
            staged[:at].copy_(pinned[:at], non_blocking=True)                      # the one upload
            for j, m in enumerate((mask, lu)):                                     # polygon planes are burnt into their
                if isinstance(m, PolygonSet):                                      # slots behind it, not uploaded
                    views[j] = (at, at + hw)
                    rasterize(m, (h, w), out=staged[at:at + hw].view(h, w))
                    at += hw
            d_rgbn = staged[:4 * hw].view(4, h, w)
            d_mask, d_lu = (None if v is None else staged[v[0]:v[1]].view(h, w) for v in views)
            ops.raster_cut(d_rgbn, d_mask, d_lu, S, t, census=census_dev)
            census = census_dev.cpu().numpy()             # the one read-back; the pinned buffer is free again after it
        else:
            cut = cut_raster_host(rgbn, mask, lu, S, t)
            census = cut[4]
        chosen = _selection(select, names, census, t)
        k = int(chosen.sum())
        fr = fracs(census, t)
        stats.extend({"file": names[i], "frac": fr[i] if masks == "keep" else 0.0} for i in np.flatnonzero(chosen).tolist())
        keys.append(key)
        table.extend(subtile_table(key, census, t))
        censuses.append((census, (h, w)))
        if k == 0:
            continue
        if on_gpu:
            rows.reserve(rows.at + k)
            slot = np.full(n, -1, np.int32)
            slot[chosen] = np.arange(rows.at, rows.at + k, dtype=np.int32)
            ops.raster_cut(d_rgbn, None if masks == "zero" else d_mask, d_lu, S, t, slot=torch.from_numpy(slot).to(dev),
                           out=rows.tensors, census=False)
            rows.at += k
        else:
            rows_needed = count + k
            need = rows_needed * (t * t * 6 + 8)
            if max_resident_bytes is not None and need > max_resident_bytes:
                raise ValueError(f"DevicePool: {rows_needed} samples of {t}x{t} need {need} bytes resident, "
                                 f"max_resident_bytes is {int(max_resident_bytes)} (streaming a split that does not fit is "
                                 "not supported)")
            images, msk, lnd, sums, _ = cut
            parts.append((images[chosen], np.zeros_like(msk[chosen]) if masks == "zero" else msk[chosen], lnd[chosen],
                          sums[chosen]))
            count += k
    if not keys:
        raise ValueError("DevicePool.from_rasters: no rasters")
    pool = DevicePool.__new__(DevicePool)
    pool.shards, pool.stats, pool.height, pool.width = [], stats, t, t
    if on_gpu:
        torch.cuda.current_stream(dev).synchronize()
        pool.images, pool.masks, pool.lu, pool.sums = rows.finish()
        pool.device = pool.images.device
    else:
        empty = (np.empty((0, t, t, 4), np.uint8), np.empty((0, t, t), np.uint8), np.empty((0, t, t), np.uint8),
                 np.empty(0, np.uint64))
        pool.images, pool.masks, pool.lu, pool.sums = (np.concatenate([p[j] for p in parts] + [empty[j]]) for j in range(4))
        pool.device = dev
    pool.n = len(stats)
    if record is not None:
        record.update(keys=keys, table=table, censuses=censuses)
    return pool


def raster_training_sets(items: Sequence, oversample: int = OVERSAMPLE_FACTOR, seed: int = 42, tile_size: int = 256,
                         source_dim: int = 2048, device=None, max_resident_bytes: Optional[int] = None) -> dict:
    """The two training sets of createdataset.py as pools: ``{"dead": pool, "random": pool, "table": rows, "censuses":
    [...]}``.  ``dead`` holds the status-1 sub-tiles with their masks; ``random`` holds ``oversample * len(dead)`` names
    drawn with ``np.random.default_rng(seed).choice(sorted(names), size, replace=False)`` from all sub-tile names of all
    rasters minus the dead ones (all of them when there are fewer), cut with ZERO masks and the rasters' lu, the blank
    ones dropped; ``table`` is the ``(name, frac, status)`` rows of the first pass, ``censuses`` what ``band_stats``
    takes.  ``items`` is read twice: a sequence or a re-iterable, not a generator."""
    if iter(items) is items:
        raise ValueError("raster_training_sets reads the rasters twice: pass a sequence or a re-iterable, not an iterator")
    record = {}
    kw = dict(tile_size=tile_size, source_dim=source_dim, device=device, max_resident_bytes=max_resident_bytes)
    dead = pool_from_rasters(items, select="dead", masks="keep", record=record, **kw)
    n = (int(source_dim) // int(tile_size)) ** 2
    dead_names = {s["file"] for s in dead.stats}
    others = sorted({name for key in record["keys"] for name in subtile_names(key, n)} - dead_names)
    size = min(int(oversample) * len(dead), len(others))
    drawn = set(np.random.default_rng(int(seed)).choice(others, size, replace=False).tolist()) if size else set()
    rnd = pool_from_rasters(items, select=lambda names, census: np.array([x in drawn for x in names], dtype=bool),
                            masks="zero", **kw)
    return {"dead": dead, "random": rnd, "table": record["table"], "censuses": record["censuses"]}


# ---------------------------------------------------------------------------------------------- band statistics
def _as_census(entry, S, t):
    """one element of ``band_stats``'s input -> (census, (h, w))"""
    if isinstance(entry, (np.ndarray, torch.Tensor)):
        return _census_array(entry), (S, S)
    if len(entry) == 2:
        return _census_array(entry[0]), (int(entry[1][0]), int(entry[1][1]))
    _, rgbn, _, _ = load_item(entry)
    h, w = rgbn.shape[1:]
    if (h, w) != (S, S):
        return np.zeros((0, CENSUS_COLS), np.int64), (h, w)        # skipped below; a ragged raster needs no cut
    return cut_raster_host(rgbn, None, None, S, t)[4], (h, w)


def band_stats(items_or_censuses: Iterable, source_dim: int = 2048, tile_size: int = 256,
               reference_denominator: bool = True) -> dict:
    """computestats.py:111-161 from the census alone: ``{"mean": [4], "std": [4], "subtiles": cnt}`` with x = byte / 255.
    Elements are raster items ``(key, rgbn, mask, lu)``, census tables [n,16] (of a full S x S raster) or ``(census, (h,
    w))`` pairs (items are cut on the host; the pairs are what a pool filled on the device has already read back:
    ``raster_training_sets(...)["censuses"]``).  Rasters that are not S x S, or whose bytes are all in {0, 255}, are skipped; of the rest the sub-tiles
    with min != max in band 0 count.  The sums are integers; mean and std follow in float64 with ``sum (x - m)^2 = sum x^2
    - 2 m sum x + N m^2``.  ``reference_denominator``: divide by ``cnt + 1`` as the reference does, otherwise by ``cnt``."""
    S, t = int(source_dim), int(tile_size)
    cnt, tot, tot2 = 0, [0, 0, 0, 0], [0, 0, 0, 0]
    for entry in items_or_censuses:
        census, (h, w) = _as_census(entry, S, t)
        if (h, w) != (S, S) or int(census[:, CENSUS_MID].sum()) == 0:
            continue
        rows = census[census[:, CENSUS_B0MIN] != census[:, CENSUS_B0MAX]]
        cnt += len(rows)
        for c in range(4):
            tot[c] += int(rows[:, CENSUS_SUM + c].sum())
            tot2[c] += int(rows[:, CENSUS_SUMSQ + c].sum())
    den = cnt + 1 if reference_denominator else cnt
    if den == 0:
        raise ValueError("band_stats: no sub-tile counts (every raster was skipped or blank in band 0)")
    N = float(t * t)
    mean, std = [], []
    for c in range(4):
        sx, sxx = tot[c] / 255.0, tot2[c] / 65025.0
        m = sx / N / den
        var = (sxx - 2.0 * m * sx + cnt * N * m * m) / N / den
        mean.append(m)
        std.append(float(np.sqrt(max(var, 0.0))))
    return {"mean": mean, "std": std, "subtiles": cnt}


def write_band_stats_json(path, stats: dict, sources: Sequence = (), frac: float = 1.0) -> dict:
    """``processed.images.stats.json`` of computestats.py:172-183: ``results`` is ``{band: {"mean", "std"}}`` for red,
    green, blue, nir.  Returns what was written."""
    info = {"sources": [str(s) for s in sources], "date": str(datetime.datetime.now()), "frac": frac,
            "subtiles": int(stats["subtiles"]),
            "results": {b: {"mean": float(stats["mean"][i]), "std": float(stats["std"][i])} for i, b in enumerate(BANDS)}}
    with open(str(path), "w") as f:
        f.write(json.dumps(info, indent=4))
    return info
