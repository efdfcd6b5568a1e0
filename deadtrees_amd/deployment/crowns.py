"""Crowns: touching dead crowns split by their inscribed depth.  A patch (``deployment/patches.py``) is a maximal connected
set of one class, so two crowns that touch are one patch and one table row; users of dead-tree maps count crowns.  The split
below cuts a patch at its necks — where its depth, the distance to the nearest pixel of another class, falls below a
threshold — and hands back a plane under the LABEL CONTRACT of ``patches.py``, so that the patch table, outlines, overlaps,
distances, gaps and attributes become crown-level with no change of their own.

The contract, in one place (the device path, ``csrc/crowns.hip`` through ``ops.patch_depth2`` /
``ops.split_patches``, computes exactly this; the functions below are the CPU path and the tests' oracle).  Everything is an
integer; device and host compare with ``array_equal``.

Inputs: a uint8 class map ``cls [h, w]`` with values ``< K``, ``2 <= K <= 8``; ``connectivity`` 4 or 8; the map's label plane
``LP`` (``label_patches``, after the sieve if any); ``CrownConfig(min_core2=E, max_rounds=256, depth_cap2=65535)``.  Sides
``<= 16384``, ``h * w <= 2**31 - 2``.

1. **Depth.**  For a pixel ``p`` with ``cls[p] = c >= 1``: ``depth2[p] = min(cap2, min over q INSIDE the raster with
   cls[q] != c of (yp - yq)**2 + (xp - xq)**2)``; ``cap2`` when there is no such ``q``; 0 on class 0.  Pixels outside the
   raster do not count: a crown cut by the raster edge keeps its core.  int32 ``[h, w]``.
2. **Cores.**  ``core[p] = cls[p]`` if ``depth2[p] >= E`` else 0; ``LC = label_patches(core, K, connectivity)``.
3. **Growth in Jacobi rounds.**  ``S_0 = LC``.  In round ``t = 1 .. max_rounds`` every pixel with ``cls != 0`` and
   ``S_{t-1} = 0`` looks at its neighbours (per ``connectivity``) of the same class with ``S_{t-1} != 0`` and, if there are
   any, takes the MINIMUM of their ``S_{t-1}``.  All pixels of a round read ``S_{t-1}`` only.  A round that changes nothing
   ends the loop: later rounds would be no-ops, so the result does not depend on when the loop stops.
4. **Remainder.**  ``rem[p] = cls[p]`` where ``S = 0``, else 0; ``LR = label_patches(rem, K, connectivity)``; ``seg = S``
   where ``S != 0``, else ``LR``.  The ids are disjoint: each names a pixel of its own set.
5. **Canonical labels.**  ``crowns[p] = 1 + min{q : seg[q] = seg[p]}``, 0 on class 0: a crown's label again names its first
   pixel in row-major order.
6. ``converged`` is true iff no pixel with ``S = 0`` and ``cls != 0`` has a same-class neighbour with ``S != 0``.  Then every
   patch that holds a core is partitioned among its cores and every patch without one is one crown with its old label.
   Before convergence the unreached parts are crowns of their own: deterministic and reported, not an error.

Every crown lies in one patch, has one class and is connected at ``connectivity``; ``E = 1`` gives ``LP``, and so does an
``E`` above the map's largest depth.

numpy only; ``scipy.ndimage`` is imported lazily (``depth2_host``, ``label_patches_host``).
"""
from __future__ import annotations

import math
from fractions import Fraction
from typing import Optional

import numpy as np

from .patches import PatchConfig, PatchTable, _check_labels, _check_map, label_patches_host, measure_patches_host
from .stats import MAX_CLASSES

MAX_SIDE = 16384
MAX_DEPTH2 = 2 ** 30
_BIG = np.int32(2 ** 31 - 1)


def _integer(value) -> bool:
    return not isinstance(value, bool) and isinstance(value, (int, np.integer))


class CrownConfig:
    """what ``crowns=`` / ``against_crowns=`` are asked for: ``min_core2`` (E) — a pixel belongs to a core when the squared
    distance to the nearest pixel of another class is at least E —, ``max_rounds`` >= 0 growth rounds, ``depth_cap2`` — the
    depth is measured up to this squared distance.  ``1 <= min_core2 <= depth_cap2 <= 2**30``, integers"""

    def __init__(self, min_core2: int, max_rounds: int = 256, depth_cap2: int = 65535):
        if not _integer(depth_cap2) or not 1 <= depth_cap2 <= MAX_DEPTH2:
            raise ValueError(f"CrownConfig: depth_cap2 must be an integer in 1..2**30, got {depth_cap2!r}")
        if not _integer(min_core2) or not 1 <= min_core2 <= depth_cap2:
            raise ValueError(f"CrownConfig: min_core2 must be an integer in 1..depth_cap2 = {int(depth_cap2)}, got "
                             f"{min_core2!r}")
        if not _integer(max_rounds) or max_rounds < 0:
            raise ValueError(f"CrownConfig: max_rounds must be an integer >= 0, got {max_rounds!r}")
        self.min_core2 = int(min_core2)
        self.max_rounds = int(max_rounds)
        self.depth_cap2 = int(depth_cap2)

    @classmethod
    def from_radius(cls, radius, max_rounds: int = 256, depth_cap2: int = 65535) -> "CrownConfig":
        """``min_core2 = ceil(radius**2)``, exactly (``Fraction``): a core pixel is at least ``radius`` pixels deep"""
        if isinstance(radius, bool) or not isinstance(radius, (int, float, Fraction, np.integer, np.floating)):
            raise ValueError(f"CrownConfig.from_radius: radius must be a number > 0, got {radius!r}")
        if not radius > 0 or (isinstance(radius, (float, np.floating)) and not math.isfinite(radius)):
            raise ValueError(f"CrownConfig.from_radius: radius must be a finite number > 0, got {radius!r}")
        r = Fraction(int(radius)) if isinstance(radius, (int, np.integer)) else Fraction(radius)
        return cls(math.ceil(r * r), max_rounds, depth_cap2)

    def __eq__(self, other) -> bool:
        if not isinstance(other, CrownConfig):
            return NotImplemented
        return ((self.min_core2, self.max_rounds, self.depth_cap2)
                == (other.min_core2, other.max_rounds, other.depth_cap2))

    __hash__ = None

    def __repr__(self) -> str:
        return f"CrownConfig(min_core2={self.min_core2}, max_rounds={self.max_rounds}, depth_cap2={self.depth_cap2})"


def check_crowns(crowns, name: str = "crowns") -> Optional[CrownConfig]:
    """the ``crowns`` / ``against_crowns`` argument of ``infer_tile`` / ``Tiler.stats`` -> ``CrownConfig`` or None (None /
    False: not asked for; True: ``CrownConfig.from_radius(2)``); anything else is a ``ValueError``"""
    if crowns is None or crowns is False:
        return None
    if crowns is True:
        return CrownConfig.from_radius(2)
    if isinstance(crowns, CrownConfig):
        return crowns
    raise ValueError(f"{name} must be True, False, None or a CrownConfig, got {crowns!r}")


def _check_classes(classes_u8, K, what: str) -> np.ndarray:
    K = int(K)
    if not 2 <= K <= MAX_CLASSES:
        raise ValueError(f"{what}: K must be in 2..{MAX_CLASSES}, got {K}")
    c = _check_map(classes_u8, what)
    if max(c.shape) > MAX_SIDE:
        raise ValueError(f"{what}: raster {c.shape}: sides must be <= {MAX_SIDE}")
    if int(c.max()) >= K:
        raise ValueError(f"{what}: class value {int(c.max())} out of range (K={K})")
    return c


def depth2_host(classes_u8, K: int, cap2: int = 65535) -> np.ndarray:
    """step 1 of the contract: int32 [h, w].  Per class ``scipy.ndimage.distance_transform_edt`` of its mask (the distance to
    the nearest pixel off the mask, exact in float64 for these sides), squared and rounded; a class that fills the raster has
    no such pixel — scipy would measure to a phantom one — and is ``cap2`` everywhere"""
    from scipy import ndimage
    c = _check_classes(classes_u8, K, "depth2")
    if not _integer(cap2) or not 1 <= cap2 <= MAX_DEPTH2:
        raise ValueError(f"depth2: cap2 must be an integer in 1..2**30, got {cap2!r}")
    out = np.zeros(c.shape, np.int32)
    for k in range(1, int(K)):
        mask = c == k
        if not mask.any():
            continue
        if mask.all():
            out[...] = cap2
            break
        d = ndimage.distance_transform_edt(mask)
        d2 = np.minimum(np.rint(d * d).astype(np.int64), int(cap2))
        out[mask] = d2[mask]
    return out


def _shifts(connectivity: int):
    if connectivity not in (4, 8) or isinstance(connectivity, bool):
        raise ValueError(f"split_patches: connectivity must be 4 or 8, got {connectivity!r}")
    near = [(-1, 0), (0, -1), (0, 1), (1, 0)]
    return near + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])


def _offers(c: np.ndarray, S: np.ndarray, shifts) -> np.ndarray:
    """int32 [h, w]: per pixel the minimum of ``S`` over its neighbours of the pixel's own class with ``S != 0``, ``_BIG``
    without one (and on pixels that are not waiting: class 0, or ``S != 0`` already)"""
    h, w = c.shape
    cp = np.zeros((h + 2, w + 2), np.uint8)
    sp = np.zeros((h + 2, w + 2), np.int32)
    cp[1:-1, 1:-1], sp[1:-1, 1:-1] = c, S
    best = np.full((h, w), _BIG, np.int32)
    for dy, dx in shifts:
        nc, ns = cp[1 + dy:1 + dy + h, 1 + dx:1 + dx + w], sp[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
        np.minimum(best, np.where((nc == c) & (ns != 0), ns, _BIG), out=best)
    best[(c == 0) | (S != 0)] = _BIG
    return best


def grow_host(classes_u8, cores, connectivity: int, max_rounds: int):
    """step 3 of the contract from ``S_0 = cores`` (int32 [h, w]): ``(S, rounds, converged)`` — ``rounds`` counts the rounds
    that labelled a pixel"""
    c, S, shifts = np.asarray(classes_u8), np.array(cores, dtype=np.int32), _shifts(connectivity)
    rounds = 0
    while True:
        offer = _offers(c, S, shifts)
        take = offer != _BIG
        if not take.any():
            return S, rounds, True
        if rounds == max_rounds:
            return S, rounds, False
        S[take] = offer[take]
        rounds += 1


def canonical_host(seg: np.ndarray) -> np.ndarray:
    """step 5 of the contract: every id of ``seg`` replaced by 1 + the row-major index of its first pixel"""
    flat = seg.ravel()
    at = np.flatnonzero(flat)                                      # ascending: the first hit of an id is its minimum
    out = np.zeros(flat.shape, np.int32)
    if len(at):
        _, first, inverse = np.unique(flat[at], return_index=True, return_inverse=True)
        out[at] = (at[first][inverse] + 1).astype(np.int32)
    return out.reshape(seg.shape)


def split_patches_host(classes_u8, labels, K: int, connectivity: int, config: CrownConfig, return_rounds: bool = False):
    """the module's contract in numpy / scipy: ``(crowns int32 [h, w], depth2 int32 [h, w], converged)``; with
    ``return_rounds`` a fourth item, the number of growth rounds that labelled a pixel.  ``labels`` is ``LP``, the label plane
    of ``classes_u8`` (a ``ValueError`` when the two do not belong together)"""
    if not isinstance(config, CrownConfig):
        raise ValueError(f"split_patches: config must be a CrownConfig, got {config!r}")
    c = np.ascontiguousarray(_check_classes(classes_u8, K, "split_patches"))
    lab = _check_labels(labels, c.shape, "split_patches")
    if ((lab != 0) != (c != 0)).any():
        raise ValueError("split_patches: labels and classes do not belong together")
    _shifts(connectivity)
    depth2 = depth2_host(c, K, config.depth_cap2)
    core = np.where(depth2 >= config.min_core2, c, 0).astype(np.uint8)
    S, rounds, converged = grow_host(c, label_patches_host(core, K, connectivity), connectivity, config.max_rounds)
    rem = np.where(S == 0, c, 0).astype(np.uint8)
    seg = np.where(S != 0, S, label_patches_host(rem, K, connectivity))
    out = (canonical_host(seg), depth2, converged)
    return out + (rounds,) if return_rounds else out


def crown_depths_host(crowns, depth2) -> np.ndarray:
    """int32 [h * w]: at every crown's root (label - 1) the largest ``depth2`` of its pixels, 0 elsewhere — the plane
    ``ops.split_patches`` returns third"""
    flat, d = np.asarray(crowns).ravel(), np.asarray(depth2).ravel()
    out = np.zeros(flat.shape, np.int32)
    at = np.flatnonzero(flat)
    np.maximum.at(out, flat[at] - 1, d[at])
    return out


class CrownSplit:
    """what a split did, aligned with the crown table ``table`` (one entry per row); numpy only and read-only.
    ``parent_root`` int64 [n]: ``LP[root] - 1``, the root of the patch a crown was cut from; ``depth2`` int32 [n]: the
    largest ``depth2`` of the crown's pixels (``radius()``: its square root, the inscribed radius in pixels); ``n_patches``:
    the patches before the split; ``converged``: step 6 of the contract; ``config``: the ``CrownConfig``"""

    def __init__(self, table: PatchTable, parent_root, depth2, converged: bool, config: CrownConfig):
        if not isinstance(table, PatchTable):
            raise ValueError("CrownSplit: table must be a PatchTable")
        if not isinstance(config, CrownConfig):
            raise ValueError(f"CrownSplit: config must be a CrownConfig, got {config!r}")
        self.table, self.config, self.converged = table, config, bool(converged)
        for name, v, dtype in (("parent_root", parent_root, np.int64), ("depth2", depth2, np.int32)):
            v = np.array(v, dtype=dtype)
            if v.shape != (table.n,):
                raise ValueError(f"CrownSplit: {name} must hold one entry per crown ({table.n}), got shape {v.shape}")
            v.setflags(write=False)
            setattr(self, "_" + name, v)
        if ((self._parent_root < 0) | (self._parent_root > table.root)).any() or (self._depth2 < 0).any():
            raise ValueError("CrownSplit: a crown's patch starts at or before the crown's own root; depths are >= 0")

    parent_root = property(lambda self: self._parent_root)
    depth2 = property(lambda self: self._depth2)

    @property
    def n(self) -> int:
        return self.table.n

    @property
    def n_patches(self) -> int:
        return len(np.unique(self._parent_root))

    def radius(self) -> np.ndarray:
        """float64 [n]: ``sqrt(depth2)``, the crown's inscribed radius in pixels (capped at ``sqrt(depth_cap2)``)"""
        return np.sqrt(self._depth2.astype(np.float64))

    def __eq__(self, other) -> bool:
        if not isinstance(other, CrownSplit):
            return NotImplemented
        return (self.table == other.table and self.config == other.config and self.converged == other.converged
                and np.array_equal(self._parent_root, other._parent_root) and np.array_equal(self._depth2, other._depth2))

    __hash__ = None

    def __repr__(self) -> str:
        return (f"CrownSplit(n={self.n}, n_patches={self.n_patches}, converged={self.converged}, "
                f"min_core2={self.config.min_core2})")


def crown_split_of(table: PatchTable, labels_before, crowns, depth2, converged: bool, config: CrownConfig) -> CrownSplit:
    """the ``CrownSplit`` of host planes: ``labels_before`` is ``LP``, ``crowns`` the crown plane ``table`` was measured on"""
    root = table.root
    return CrownSplit(table, np.asarray(labels_before).ravel()[root].astype(np.int64) - 1,
                      crown_depths_host(crowns, depth2)[root], converged, config)


def crowned_patches_host(classes_u8, labels, K: int, connectivity: int, config: CrownConfig):
    """split -> measure on the host: ``(crowns, PatchTable of the crowns, CrownSplit)``"""
    crowns, depth2, converged = split_patches_host(classes_u8, labels, K, connectivity, config)
    table = measure_patches_host(crowns, classes_u8)
    return crowns, table, crown_split_of(table, labels, crowns, depth2, converged, config)


def split_patches(map_or_polygons, K: int, config: CrownConfig, connectivity: int = 8, device=None, shape=None):
    """the stand-alone entry, taking its map as ``overlaps.patch_overlaps`` does (a uint8 class map, array or tensor, or a
    ``PolygonSet`` in pixel coordinates with ``shape``, burnt with ``all_touched=True``): label -> split -> table.  Returns
    ``(crowns, CrownSplit)``: the crown plane — a host array, or a tensor on the ``cuda`` device the work ran on — and the
    split, whose ``table`` is the crown table.  The input is not written"""
    from .overlaps import checked_maps
    if not isinstance(config, CrownConfig):
        raise ValueError(f"split_patches: config must be a CrownConfig, got {config!r}")
    patches = PatchConfig(connectivity)
    (plane,), _, dev = checked_maps("split_patches", (map_or_polygons,), K, (patches,), device, shape)
    if dev is None:
        from .patches import labelled_patches_host
        _, crowns, _, split = labelled_patches_host(plane, int(K), patches, crowns=config)
        return crowns, split
    import torch
    from .analysis import device_patches
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    crowns, _, split = device_patches(plane, int(K), patches, err, crowns=config)
    if int(err.cpu()):
        raise ValueError(f"split_patches: class value out of range (K={int(K)})")
    return crowns, split


__all__ = ["CrownConfig", "CrownSplit", "check_crowns", "depth2_host", "grow_host", "canonical_host", "split_patches_host",
           "crown_depths_host", "crown_split_of", "crowned_patches_host", "split_patches"]
