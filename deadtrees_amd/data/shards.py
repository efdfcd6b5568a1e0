"""Webdataset shards without the ``webdataset`` package: reader, train/val/test split, per-rank assignment.

The reference streams ``*.tar`` shards through ``wds.WebDataset(...).map(sample_decoder)`` every epoch
(deadtrees/data/deadtreedata.py:91-125, 263-288).  Here a shard is read ONCE with the stdlib ``tarfile`` into uint8 arrays
that ``data/pool.py`` keeps resident on the device.  A sample is the run of consecutive members that share a key — the
member path up to the first ``.`` of its basename; the rest is the field name: ``a/b.rgbn.tif`` is field ``rgbn.tif`` of
sample ``a/b``.  Fields: ``rgbn.tif`` (decoded as RGBA, so a 3-band file gets 255 as its fourth band), ``mask.tif`` and
``lu.tif`` (decoded as L) and ``txt`` (the dead-tree fraction).
"""
from __future__ import annotations

import io
import logging
import os
import tarfile
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, List, Optional, Sequence

import numpy as np

logger = logging.getLogger(__name__)

IMG, MSK, LU, TXT = "rgbn.tif", "mask.tif", "lu.tif", "txt"
FIELDS = (IMG, MSK, LU, TXT)
MAX_DECODE_WORKERS = 16      # a fixed cap: the machine's CPU count says nothing about this process's share of it


def split_key(name: str):
    """webdataset's ``base_plus_ext``: ``dir/base.ext1.ext2`` -> (``dir/base``, ``ext1.ext2``); no ``.`` -> (None, None)"""
    head, base = os.path.split(name)
    if "." not in base:
        return None, None
    stem, field = base.split(".", 1)
    return (head + "/" + stem if head else stem), field


def _group(tar: tarfile.TarFile):
    """[(key, {field: TarInfo})] — consecutive members with one key make one sample (webdataset's ``group_by_keys``)"""
    samples, key, cur = [], None, None
    for m in tar:
        if not m.isreg():
            continue
        k, field = split_key(m.name)
        if k is None:
            continue
        if k != key:
            key, cur = k, {}
            samples.append((k, cur))
        cur[field.lower()] = m
    return samples


def shard_len(path) -> int:
    """number of samples of a shard (reads the member headers only)"""
    with tarfile.open(str(path), "r:*") as tar:
        return len(_group(tar))


def _decode(data: bytes, mode: str) -> np.ndarray:
    from PIL import Image
    with io.BytesIO(data) as stream:
        img = Image.open(stream)
        img.load()
        img = img.convert(mode)
    return np.asarray(img)


def read_shard(path, alloc: Optional[Callable] = None, workers: int = 8) -> dict:
    """One shard -> {"images": uint8 [n,H,W,4], "masks": uint8 [n,H,W], "lu": uint8 [n,H,W], "sums": uint64 [n],
    "stats": [{"file": key, "frac": float}], "keys": [key]} in member order.  ``sums[i]`` is the exact sum of all 4*H*W
    bytes of image i.  ``alloc(shape, dtype)`` supplies the three big arrays (the pool hands out pinned memory); default
    ``np.empty``.  Raises ``ValueError`` naming shard and key for a sample that lacks a field, whose tile size differs
    from the first sample's, or whose H or W is no multiple of 32 (the network's five stride-2 stages)."""
    path = str(path)
    alloc = alloc or (lambda shape, dtype: np.empty(shape, dtype))
    with tarfile.open(path, "r:*") as tar:
        samples = _group(tar)
        if not samples:
            raise ValueError(f"{path}: no samples")
        raw = []
        for key, members in samples:       # one reader: a TarFile is not safe to read from several threads
            missing = [f for f in FIELDS if f not in members]
            if missing:
                raise ValueError(f"{path}: sample {key!r} has no {', '.join(missing)}")
            raw.append({f: tar.extractfile(members[f]).read() for f in FIELDS})
    n = len(samples)
    first = _decode(raw[0][IMG], "RGBA")
    H, W = first.shape[:2]
    if H % 32 or W % 32:
        raise ValueError(f"{path}: sample {samples[0][0]!r} is {H}x{W}; tile height and width must be multiples of 32")
    images, masks, lu = alloc((n, H, W, 4), np.uint8), alloc((n, H, W), np.uint8), alloc((n, H, W), np.uint8)
    sums = np.empty(n, np.uint64)
    stats: List[Optional[dict]] = [None] * n

    def one(i):
        key = samples[i][0]
        for field, mode, dst in ((IMG, "RGBA", images), (MSK, "L", masks), (LU, "L", lu)):
            arr = first if (i == 0 and field == IMG) else _decode(raw[i][field], mode)
            if arr.shape[:2] != (H, W):
                raise ValueError(f"{path}: {field} of sample {key!r} is {arr.shape[0]}x{arr.shape[1]}, "
                                 f"the shard's first tile is {H}x{W}")
            dst[i] = arr
        sums[i] = images[i].sum(dtype=np.uint64)
        stats[i] = {"file": key, "frac": float(raw[i][TXT].decode())}      # sample_decoder, :116-117

    with ThreadPoolExecutor(max_workers=max(1, min(int(workers), MAX_DECODE_WORKERS, n))) as pool:
        list(pool.map(one, range(n)))          # (re-raises the first error)
    return {"images": images, "masks": masks, "lu": lu, "sums": sums, "stats": stats, "keys": [k for k, _ in samples]}


def split_shards(original_list, split_fractions):
    """Distribute shards into train / valid / test parts (reference deadtreedata.py:47-88, quirks kept): cut points are
    ``int(round(n * w))`` (Python's round-half-even) on the sorted list, slices truncate at its end, and a split with an
    empty part is repaired — three-way to ``[:-2], [-2:-1], [-1:]`` if the first part holds more than 2 shards (else
    ``ValueError``), two-way to ``[:-1], [-1:]``.  A two-way split returns ``None`` as its third part."""
    total = float(sum(split_fractions))
    assert np.isclose(total, 1.0), f"split fractions sum to {total}, not 1"
    shards = [str(p) for p in sorted(original_list)]
    n, ways = len(shards), len(split_fractions)
    if ways not in (2, 3):
        raise ValueError(f"a split has 2 or 3 parts, not {ways}")
    cuts = np.concatenate([[0], np.cumsum([int(round(n * f)) for f in split_fractions])])
    parts = [shards[a:b] for a, b in zip(cuts[:-1], cuts[1:])]      # (a slice past the end is just shorter)
    assert sum(map(len, parts)) == n, f"split sizes {[len(p) for p in parts]} do not add up to {n} shards"
    if min(map(len, parts)) == 0:
        if ways == 3 and len(parts[0]) <= 2:
            raise ValueError(f"{n} shards are too few for a train / valid / test split")
        tail = ways - 1
        parts = [shards[:-tail]] + [[s] for s in shards[-tail:]]    # one shard each for the last part(s)
        logger.warning("a part of the shard split was empty; repaired to sizes %s", [len(p) for p in parts])
    return parts if ways == 3 else parts + [None]


def shards_for_rank(shards: Sequence, rank: int, world: int) -> list:
    """data-parallel assignment: shard i belongs to rank ``i % world``; a rank without a shard cannot train"""
    if world < 1 or not 0 <= rank < world:
        raise ValueError(f"rank {rank} of world {world}")
    mine = [s for i, s in enumerate(shards) if i % world == rank]
    if not mine:
        raise ValueError(f"rank {rank} of {world} gets none of the {len(shards)} shards")
    return mine
