"""Nearest-patch distances: how far is every patch from the patches of another map — the spread distance of this year's
new dead trees from last year's — and how far from the OTHER patches of its own map, the nearest-neighbour gap that every
clustering index starts from.  ``PatchOverlaps`` is defined on shared pixels and says nothing about either.

The contract, in one place (the device path, ``csrc/proximity.hip`` through ``ops.patch_proximity``, computes
exactly this; ``patch_proximity_host`` is the CPU path):

* ``LS`` (source) and ``LQ`` (query) are two int32 ``[h, w]`` label planes on the same grid, each under the contract of
  ``deployment/patches.py``: 0 on background, elsewhere ``1 + root``.  Connectivity, K and sieve may differ;
* ``d2(p, q) = (yp - yq)**2 + (xp - xq)**2`` between pixel centres: an integer;
* for the query patch ``b`` (a root of ``LQ``) take the pairs ``(p, q)`` with ``LQ[p] == 1 + b``, ``LS[q] != 0``, in
  ``exclude_own`` mode ``LS[q] != LQ[p]``, and with a limit ``d2(p, q) <= limit2``.  The result is the lexicographic minimum
  of ``(d2(p, q), LS[q] - 1)`` over them: ``d2[b]`` the smallest squared distance and ``nearest[b]`` the SMALLEST root among
  the source patches that reach it, both int64 and both ``-1`` without such a pair;
* the result is unique: it depends on no traversal order, so device and host compare with ``array_equal``;
* ``limit2 = floor(max_distance**2)`` (``ProximityConfig.limit2``); a pair at exactly ``limit2`` counts;
* sides <= 16384 and ``h * w <= 2**31 - 2``.

Two uses of the one rule.  *Between* two maps (``patch_distances``, ``infer_tile(..., distances=...)``), run in both
directions: a patch that shares a pixel with the other map has ``d2 == 0``.  *Within* one map (``patch_gaps``,
``infer_tile(..., gaps=...)``; ``exclude_own`` with ``LS is LQ``): patches of different classes that touch have ``d2 == 1``,
diagonal neighbours under connectivity 4 have ``d2 == 2``.

The search is separable, on both paths: a source pixel at minimum distance from ``p`` is the nearest admissible pixel of its
own column above or below ``p``'s row, so per column and vertical direction the nearest labelled pixel is tabled once (for
``exclude_own`` also the nearest one whose label differs from that: a query takes the first that is not its own), and a
query pixel minimises ``(dx**2 + g**2, label)`` over the columns of its row, outward while ``dx**2`` can still win.

numpy and the standard library only.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from .patches import MAX_PIXELS, PatchConfig, PatchTable

MAX_SIDE = 16384
_NONE = np.int64(1) << 62        # a key above every (d2 << 32 | root)


@dataclass(frozen=True)
class ProximityConfig:
    """what ``distances=`` / ``gaps=`` are asked for: ``max_distance`` in pixels (>= 0; None: no limit) — a patch farther
    than that from everything has no nearest patch.  ``limit2 = floor(max_distance**2)``, None without a limit"""
    max_distance: Optional[float] = None

    def __post_init__(self):
        m = self.max_distance
        if m is not None and (isinstance(m, bool) or not isinstance(m, (int, float, np.integer, np.floating))
                              or not m >= 0 or math.isinf(m)):
            raise ValueError(f"ProximityConfig: max_distance must be a finite number >= 0 or None, got {m!r}")

    @property
    def limit2(self) -> Optional[int]:
        m = self.max_distance
        if m is None:
            return None
        return int(m) * int(m) if isinstance(m, (int, np.integer)) else int(math.floor(float(m) * float(m)))


def check_proximity(option, name: str) -> Optional[ProximityConfig]:
    """the ``distances`` / ``gaps`` argument of ``infer_tile`` -> ``ProximityConfig`` or None (None / False: not asked for;
    True: no limit); anything else is a ``ValueError``"""
    if option is None or option is False:
        return None
    if option is True:
        return ProximityConfig()
    if isinstance(option, ProximityConfig):
        return option
    raise ValueError(f"{name} must be True, False, None or a ProximityConfig, got {option!r}")


def _check_limit2(limit2) -> Optional[int]:
    if limit2 is None:
        return None
    if isinstance(limit2, bool) or int(limit2) != limit2 or limit2 < 0:
        raise ValueError(f"patch_proximity: limit2 must be an integer >= 0 or None, got {limit2!r}")
    return int(limit2)


def _column_tables(ls: np.ndarray):
    """per pixel the nearest labelled pixel of its column at or above its row, ``(g1, l1)``, and the nearest one at or above
    whose label differs from ``l1``, ``(g2, l2)``: row distances int64 (-1: none) and labels"""
    h, w = ls.shape
    rows = np.arange(h, dtype=np.int64)[:, None]
    cols = np.arange(w)[None, :]
    labelled = ls > 0
    r1 = np.maximum.accumulate(np.where(labelled, rows, -1), axis=0)
    l1 = np.where(r1 >= 0, ls[np.maximum(r1, 0), cols], 0)
    # the labelled pixel strictly above every row, and the rows where a stretch of one label starts: the state changes there
    before_r = np.vstack([np.full((1, w), -1, np.int64), r1[:-1]])
    before_l = np.vstack([np.zeros((1, w), ls.dtype), l1[:-1]])
    starts = labelled & (before_l != ls)
    at = np.maximum.accumulate(np.where(starts, rows, -1), axis=0)
    r2 = np.where(at >= 0, before_r[np.maximum(at, 0), cols], -1)
    l2 = np.where(r2 >= 0, before_l[np.maximum(at, 0), cols], 0)
    return np.where(r1 >= 0, rows - r1, -1), l1, np.where(r2 >= 0, rows - r2, -1), l2


def patch_proximity_host(labels_src, labels_qry, roots_qry, exclude_own: bool = False, limit2=None):
    """the module's contract in numpy: int64 arrays ``(d2, nearest_root)``, one entry per element of ``roots_qry`` (the
    ascending roots of the query plane's table).  ``ValueError`` for a dtype other than int32, unequal shapes, an empty plane,
    a side above 16384 and a ``limit2`` that is no integer >= 0.  Exact: column tables by running maxima, then all query
    pixels step outward along their rows together, each as long as ``dx**2`` does not exceed what it, or its patch, has.
    Between two planes scipy's exact Euclidean feature transform (when scipy is there) first gives every query pixel's own
    d2, so that only the pixels at their patch's minimum walk, and no farther than it: they settle which root it is"""
    ls, lq = np.asarray(labels_src), np.asarray(labels_qry)
    if ls.dtype != np.int32 or lq.dtype != np.int32:
        raise ValueError(f"patch_proximity: labels must be int32, got {ls.dtype} and {lq.dtype}")
    if ls.ndim != 2 or ls.shape != lq.shape:
        raise ValueError(f"patch_proximity: the label planes must be [h, w] on one grid, got {ls.shape} and {lq.shape}")
    if ls.size == 0 or max(ls.shape) > MAX_SIDE or ls.size > MAX_PIXELS:
        raise ValueError(f"patch_proximity: planes of {ls.shape}: sides must be in 1..{MAX_SIDE}, h * w <= {MAX_PIXELS}")
    limit2 = _check_limit2(limit2)
    roots = np.asarray(roots_qry).astype(np.int64).ravel()
    n, (h, w) = len(roots), ls.shape
    best = np.full(n, _NONE, np.int64)
    qy, qx = np.nonzero(lq > 0)
    own = lq[qy, qx].astype(np.int64)
    row = np.searchsorted(roots, own - 1)
    known = (row < n) & (roots[np.minimum(row, max(n - 1, 0))] == own - 1) if n else np.zeros(len(own), bool)
    qy, qx, own, row = qy[known], qx[known], own[known], row[known]
    if n and len(qy) and (ls > 0).any():
        tables = [_column_tables(ls), tuple(t[::-1] for t in _column_tables(ls[::-1]))]      # at or above, at or below
        bound = np.full(len(qy), np.int64(2) ** 31 if limit2 is None else min(limit2, 2 ** 31), np.int64)
        if not exclude_own:
            qy, qx, own, row, bound = _patch_minima(ls, qy, qx, own, row, bound, n)
        key = np.full(len(qy), _NONE, np.int64)
        active = np.arange(len(qy))
        for dx in range(w):
            reach = np.minimum(bound[active], best[row[active]] >> 32)
            active = active[(dx * dx <= reach) & ((qx[active] >= dx) | (qx[active] + dx < w))]
            if not len(active):
                break
            for side in ((-dx, dx) if dx else (0,)):
                xx = qx[active] + side
                inside = (xx >= 0) & (xx < w)
                i, yy, xx = active[inside], qy[active[inside]], xx[inside]
                for g1, l1, g2, l2 in tables:
                    g, label = g1[yy, xx], l1[yy, xx].astype(np.int64)
                    if exclude_own:
                        mine = label == own[i]
                        g, label = np.where(mine, g2[yy, xx], g), np.where(mine, l2[yy, xx], label)
                    d2 = dx * dx + g * g
                    ok = (g >= 0) & (d2 <= bound[i])
                    key[i] = np.minimum(key[i], np.where(ok, (d2 << 32) | (label - 1), _NONE))
            bound[active] = np.minimum(bound[active], key[active] >> 32)
            np.minimum.at(best, row[active], key[active])
    none = best == _NONE
    return np.where(none, -1, best >> 32), np.where(none, -1, best & 0xffffffff)


def _patch_minima(ls, qy, qx, own, row, bound, n):
    """the query pixels that reach their patch's smallest d2 to a labelled pixel of ``ls`` within their ``bound``, with that d2
    as their bound — from scipy's feature transform, whose indices give d2 in integers; everything unchanged without scipy"""
    try:
        from scipy.ndimage import distance_transform_edt
    except ImportError:
        return qy, qx, own, row, bound
    at = distance_transform_edt(ls <= 0, return_distances=False, return_indices=True)
    d2 = (at[0][qy, qx].astype(np.int64) - qy) ** 2 + (at[1][qy, qx].astype(np.int64) - qx) ** 2
    least = np.full(n, _NONE, np.int64)
    np.minimum.at(least, row, d2)
    keep = (d2 == least[row]) & (d2 <= bound)
    return qy[keep], qx[keep], own[keep], row[keep], d2[keep]


def _nearest_rows(table: PatchTable, nearest_root: np.ndarray, what: str) -> np.ndarray:
    """roots of ``table`` (-1: none) -> its rows (-1: none); a root the table does not have is a ``ValueError``"""
    rows = np.full(len(nearest_root), -1, np.int64)
    some = nearest_root >= 0
    at = np.searchsorted(table.root, nearest_root[some])
    if some.any() and (table.n == 0 or (table.root[np.minimum(at, table.n - 1)] != nearest_root[some]).any()):
        raise ValueError(f"{what}: a nearest root is missing from its table")
    rows[some] = at
    return rows


def _column(v, n: int, what: str) -> np.ndarray:
    v = np.array(v, dtype=np.int64)
    if v.shape != (n,):
        raise ValueError(f"{what}: expected {n} entries, got shape {v.shape}")
    v.setflags(write=False)
    return v


def _check_side(table: PatchTable, other: PatchTable, d2, nearest, what: str):
    d2, nearest = _column(d2, table.n, what), _column(nearest, table.n, what)
    if ((d2 < -1) | (nearest < -1) | ((d2 < 0) != (nearest < 0)) | (nearest >= max(other.n, 0))).any():
        raise ValueError(f"{what}: d2 >= 0 with a row of the other table, or -1 and -1")
    return d2, nearest


def _distance(d2: np.ndarray) -> np.ndarray:
    return np.where(d2 >= 0, np.sqrt(np.maximum(d2, 0).astype(np.float64)), np.nan)


def _histogram(table: PatchTable, d2: np.ndarray, edges, weights: str, only) -> np.ndarray:
    """int64 [len(edges) + 1]: the patches — or with ``weights="area"`` their pixels — per distance band, over the patches
    that have a distance (and that ``only`` selects).  ``edges`` ascending, in pixels; bin 0 holds ``distance < edges[0]``,
    bin ``j`` ``edges[j - 1] <= distance < edges[j]``, the last ``distance >= edges[-1]``"""
    edges = np.asarray(edges, dtype=np.float64)
    if edges.ndim != 1 or len(edges) == 0 or (np.diff(edges) <= 0).any():
        raise ValueError("histogram: edges must be a non-empty ascending sequence")
    if weights not in ("count", "area"):
        raise ValueError(f"histogram: weights must be 'count' or 'area', got {weights!r}")
    take = d2 >= 0
    if only is not None:
        only = np.asarray(only)
        if only.dtype != bool or only.shape != d2.shape:
            raise ValueError(f"histogram: only must be a bool array with one entry per patch, got {only.dtype} {only.shape}")
        take = take & only
    bins = np.searchsorted(edges, _distance(d2[take]), side="right")
    amount = table.area[take] if weights == "area" else np.ones(int(take.sum()), np.int64)
    out = np.zeros(len(edges) + 1, np.int64)
    np.add.at(out, bins, amount)
    return out


class PatchDistances:
    """the nearest-patch distances of two maps, both directions, joined with their ``PatchTable``s; numpy only and
    read-only.  ``a_d2`` int64 [n_a]: per patch of A the squared distance to the nearest labelled pixel of B (0: they share
    a pixel; -1: none, or none within the limit); ``a_nearest`` int64 [n_a]: the ROW in ``table_b`` of the nearest patch
    (the smallest root among those at that distance; -1: none); ``b_d2`` / ``b_nearest`` the same for the patches of B
    against A"""

    def __init__(self, table_a: PatchTable, table_b: PatchTable, a_d2, a_nearest, b_d2, b_nearest):
        if not isinstance(table_a, PatchTable) or not isinstance(table_b, PatchTable):
            raise ValueError("PatchDistances: table_a and table_b must be PatchTables")
        if table_a.shape != table_b.shape:
            raise ValueError(f"PatchDistances: the tables lie on different grids, {table_a.shape} and {table_b.shape}")
        self.table_a, self.table_b = table_a, table_b
        self._a_d2, self._a_nearest = _check_side(table_a, table_b, a_d2, a_nearest, "PatchDistances")
        self._b_d2, self._b_nearest = _check_side(table_b, table_a, b_d2, b_nearest, "PatchDistances")

    a_d2 = property(lambda self: self._a_d2)
    a_nearest = property(lambda self: self._a_nearest)
    b_d2 = property(lambda self: self._b_d2)
    b_nearest = property(lambda self: self._b_nearest)

    @classmethod
    def from_roots(cls, table_a, table_b, a, b) -> "PatchDistances":
        """from the two ``(d2, nearest_root)`` results of ``patch_proximity``: A queried against B, and B against A"""
        return cls(table_a, table_b, a[0], _nearest_rows(table_b, np.asarray(a[1]), "PatchDistances"),
                   b[0], _nearest_rows(table_a, np.asarray(b[1]), "PatchDistances"))

    def a_distance(self) -> np.ndarray:
        """float64 [n_a]: the distance in pixels, nan for none"""
        return _distance(self._a_d2)

    def b_distance(self) -> np.ndarray:
        """float64 [n_b]: the distance in pixels, nan for none"""
        return _distance(self._b_d2)

    def a_distance_m(self, pixel_size: float = 0.2) -> np.ndarray:
        """``a_distance`` in metres, for a pixel of ``pixel_size`` metres"""
        return self.a_distance() * float(pixel_size)

    def b_distance_m(self, pixel_size: float = 0.2) -> np.ndarray:
        """``b_distance`` in metres"""
        return self.b_distance() * float(pixel_size)

    def histogram(self, edges, side: str = "b", weights: str = "count", only=None) -> np.ndarray:
        """the patches of ``side`` ("a" or "b") per distance band: see ``PatchGaps.histogram``; ``only``: a bool per patch of
        that side, such as ``overlaps.track().b_state == NEW``"""
        if side not in ("a", "b"):
            raise ValueError(f"histogram: side must be 'a' or 'b', got {side!r}")
        return _histogram(self.table_a if side == "a" else self.table_b, self._a_d2 if side == "a" else self._b_d2, edges,
                          weights, only)

    def __eq__(self, other) -> bool:
        if not isinstance(other, PatchDistances):
            return NotImplemented
        return (self.table_a == other.table_a and self.table_b == other.table_b
                and all(np.array_equal(getattr(self, c), getattr(other, c))
                        for c in ("_a_d2", "_a_nearest", "_b_d2", "_b_nearest")))

    __hash__ = None

    def __repr__(self) -> str:
        return (f"PatchDistances(n_a={self.table_a.n}, n_b={self.table_b.n}, "
                f"a: {_summary(self._a_d2)}, b: {_summary(self._b_d2)})")


def _summary(d2: np.ndarray, touching: int = 0) -> str:
    """``touching``: the d2 of two patches without a pixel between them — 0 between two maps, 1 within one"""
    some = d2[d2 >= 0]
    far = f", farthest {math.sqrt(int(some.max())):.1f} px" if len(some) else ""
    return (f"{int((some <= touching).sum())} touching, {int((some > touching).sum())} apart, {int((d2 < 0).sum())} without"
            f"{far}")


class PatchGaps:
    """the gap of every patch of ONE map to the nearest other patch of that map, aligned with its ``PatchTable``.  ``d2``
    int64 [n]: the squared distance between the nearest pixels (1: the patches touch, which patches of different classes
    can; -1: there is no other patch, or none within the limit); ``nearest`` int64 [n]: the table ROW of that patch (the
    smallest root among those at that distance; -1: none)"""

    def __init__(self, table: PatchTable, d2, nearest):
        if not isinstance(table, PatchTable):
            raise ValueError("PatchGaps: table must be a PatchTable")
        self.table = table
        self._d2, self._nearest = _check_side(table, table, d2, nearest, "PatchGaps")
        if (self._d2 == 0).any() or (self._nearest == np.arange(table.n)).any():
            raise ValueError("PatchGaps: a patch cannot be its own neighbour")

    d2 = property(lambda self: self._d2)
    nearest = property(lambda self: self._nearest)

    @classmethod
    def from_roots(cls, table, result) -> "PatchGaps":
        """from the ``(d2, nearest_root)`` of ``patch_proximity`` with ``exclude_own``"""
        return cls(table, result[0], _nearest_rows(table, np.asarray(result[1]), "PatchGaps"))

    def distance(self) -> np.ndarray:
        """float64 [n]: the gap in pixels, nan for none"""
        return _distance(self._d2)

    def distance_m(self, pixel_size: float = 0.2) -> np.ndarray:
        """``distance`` in metres, for a pixel of ``pixel_size`` metres"""
        return self.distance() * float(pixel_size)

    def histogram(self, edges, weights: str = "count", only=None) -> np.ndarray:
        """int64 [len(edges) + 1]: the patches (``weights="area"``: their pixels) per band of ``distance()`` over the patches
        that have one and that the bool array ``only`` selects.  ``edges`` ascending, in pixels; bin 0 holds ``distance <
        edges[0]``, bin ``j`` ``edges[j - 1] <= distance < edges[j]``, the last bin ``distance >= edges[-1]``"""
        return _histogram(self.table, self._d2, edges, weights, only)

    def __eq__(self, other) -> bool:
        if not isinstance(other, PatchGaps):
            return NotImplemented
        return (self.table == other.table and np.array_equal(self._d2, other._d2)
                and np.array_equal(self._nearest, other._nearest))

    __hash__ = None

    def __repr__(self) -> str:
        return f"PatchGaps(n={self.table.n}, {_summary(self._d2, 1)})"


# ---------------------------------------------------------------------------------------------- label planes in
def distances_of(labels_a, table_a: PatchTable, labels_b, table_b: PatchTable, limit2=None, device: bool = False):
    """``PatchDistances`` of two label planes and their tables: both directions of the one rule, through
    ``ops.patch_proximity`` with ``device`` (the planes are device tensors), else ``patch_proximity_host``"""
    if device:
        from ..ops import patch_proximity as run
    else:
        run = patch_proximity_host
    return PatchDistances.from_roots(table_a, table_b, run(labels_b, labels_a, table_a.root, False, limit2),
                                     run(labels_a, labels_b, table_b.root, False, limit2))


def gaps_of(labels, table: PatchTable, limit2=None, device: bool = False):
    """``PatchGaps`` of a label plane and its table (``exclude_own``), on the device or on the host like ``distances_of``"""
    if device:
        from ..ops import patch_proximity as run
    else:
        run = patch_proximity_host
    return PatchGaps.from_roots(table, run(labels, labels, table.root, True, limit2))


def _proximity(proximity, who: str) -> ProximityConfig:
    if proximity is not None and not isinstance(proximity, ProximityConfig):
        raise ValueError(f"{who}: proximity must be a ProximityConfig or None, got {proximity!r}")
    return ProximityConfig() if proximity is None else proximity


# ---------------------------------------------------------------------------------------------- maps in
def patch_distances(map_a, map_b, K: int, config_a: Optional[PatchConfig] = None, config_b: Optional[PatchConfig] = None,
                    proximity: Optional[ProximityConfig] = None, device=None, shape=None) -> PatchDistances:
    """the ``PatchDistances`` of two maps on one grid, taken as ``overlaps.patch_overlaps`` takes them: uint8 class maps
    (arrays or tensors) or ``PolygonSet``s in pixel coordinates (burnt with ``all_touched=True``); label -> (sieve) -> table
    on both (``config_a`` / ``config_b``), then the distances in both directions under ``proximity`` (default: no limit).
    On the host ``patch_proximity_host``; with device tensors, or ``device`` a ``cuda`` device, ``ops.patch_proximity`` on
    the label planes in HBM: only the tables and the result are downloaded.  Neither input is written"""
    from .overlaps import labelled_maps
    limit2 = _proximity(proximity, "patch_distances").limit2
    (labels_a, labels_b), (table_a, table_b), dev = labelled_maps("patch_distances", (map_a, map_b), K, (config_a, config_b),
                                                                  device, shape)
    return distances_of(labels_a, table_a, labels_b, table_b, limit2, dev is not None)


def patch_gaps(map, K: int, config: Optional[PatchConfig] = None, proximity: Optional[ProximityConfig] = None,
               device=None) -> PatchGaps:
    """the ``PatchGaps`` of one map (a uint8 class map, array or tensor): label -> (sieve) -> table under ``config``, then
    every patch's gap to the nearest other patch under ``proximity``.  Host or device as in ``patch_distances``"""
    from ..data.polygons import PolygonSet
    from .overlaps import labelled_maps
    if isinstance(map, PolygonSet):
        raise ValueError("patch_gaps: a PolygonSet needs a grid: burn it first (data.polygons.rasterize)")
    limit2 = _proximity(proximity, "patch_gaps").limit2
    (labels,), (table,), dev = labelled_maps("patch_gaps", (map,), K, (config,), device)
    return gaps_of(labels, table, limit2, dev is not None)
