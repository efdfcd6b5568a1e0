"""Patch overlaps: two maps on one grid compared patch by patch — the annotators' crowns against the predicted patches
(how many crowns were found, how many patches are spurious, with what IoU), or last year's map against this year's (which
patches are new, which vanished, grew, merged or split).  Both are read off ONE small table.

The contract, in one place (the device path, ``csrc/overlaps.hip`` through ``ops.patch_overlaps``, computes
exactly this; ``overlap_pairs_host`` is the CPU path and the tests' yardstick):

* ``LA`` and ``LB`` are two int32 ``[h, w]`` label planes on the same grid, each under the contract of
  ``deployment/patches.py``: 0 on background, elsewhere ``1 + root``.  The two may come from different connectivities,
  different K, sieved or not;
* the **overlap table** is the set of rows ``(a, b, n)``: ``a = LA[p] - 1`` and ``b = LB[p] - 1`` for the pixels ``p``
  where both labels are non-zero, ``n`` the number of such pixels of that pair.  Only pairs with ``n > 0`` appear; rows are
  sorted ascending by ``(a, b)``; all three columns are int64;
* the table is unique: it depends on no launch order and on no implementation choice, so device and host compare with
  ``array_equal``;
* a pair whose intersection is disconnected is still ONE row;
* pairs of different classes are rows too: class filters are applied later, on the host (``same_class``).

``PatchOverlaps`` joins the table with the two ``PatchTable``s (the areas an IoU needs); ``match`` reads the crown-level
accuracy off it and ``track`` the year-to-year fate of every patch.  A is the reference — the annotation, or the earlier
year — and B the map under test.

numpy and the standard library only (``label_patches_host`` imports scipy lazily).
"""
from __future__ import annotations

from fractions import Fraction
from typing import Optional

import numpy as np

from .patches import PatchConfig, PatchTable, labelled_patches_host
from .stats import MAX_CLASSES

VANISHED, CONTINUED, SPLIT, MERGED_INTO = 0, 1, 2, 3      # PatchTracks.a_state
NEW, MERGED, SPLIT_FROM = 0, 2, 3                          # PatchTracks.b_state (CONTINUED = 1 on both sides)
A_STATES = ("VANISHED", "CONTINUED", "SPLIT", "MERGED_INTO")
B_STATES = ("NEW", "CONTINUED", "MERGED", "SPLIT_FROM")


def overlap_pairs_host(labels_a, labels_b):
    """the module's contract in vectorised numpy: ``(a, b, n)`` int64, ascending in ``(a, b)``.  ``ValueError`` for a dtype
    other than int32, unequal shapes and an empty plane"""
    la, lb = np.asarray(labels_a), np.asarray(labels_b)
    if la.dtype != np.int32 or lb.dtype != np.int32:
        raise ValueError(f"overlap_pairs: labels must be int32, got {la.dtype} and {lb.dtype}")
    if la.ndim != 2 or la.shape != lb.shape:
        raise ValueError(f"overlap_pairs: the label planes must be [h, w] on one grid, got {la.shape} and {lb.shape}")
    if la.size == 0:
        raise ValueError("overlap_pairs: empty plane")
    la, lb = la.ravel(), lb.ravel()
    at = np.flatnonzero((la > 0) & (lb > 0))
    key, n = np.unique((la[at].astype(np.int64) << 32) | lb[at].astype(np.int64), return_counts=True)
    return (key >> 32) - 1, (key & 0xffffffff) - 1, n.astype(np.int64)


def _rows_of(table: PatchTable, roots: np.ndarray, side: str) -> np.ndarray:
    """the rows of ``roots`` in ``table``; a root the table does not have is a ``ValueError``"""
    rows = np.searchsorted(table.root, roots).astype(np.int64)
    if len(roots) and (table.n == 0 or (table.root[np.minimum(rows, table.n - 1)] != roots).any()):
        raise ValueError(f"PatchOverlaps: {side} names a root that its table does not have")
    return rows


class PatchOverlaps:
    """the overlap table of two label planes joined with their ``PatchTable``s; numpy only and read-only, like
    ``PatchTable``.  ``table_a`` / ``table_b`` (same ``shape``); ``a`` / ``b`` / ``n``: the rows of the module's contract;
    ``ia`` / ``ib`` int64: the row of each pair's patch in the two tables; ``inter`` is ``n``.  ``ValueError`` when a root
    is missing from its table, the rows are not strictly ascending in ``(a, b)``, or some ``n`` is below 1 or above
    ``min(area_a, area_b)``.  ``distances``: the ``PatchDistances`` (``deployment/proximity.py``) of the same two tables when
    they were asked for, else None — then ``repr`` and ``==`` do not mention them"""

    def __init__(self, table_a: PatchTable, table_b: PatchTable, a, b, n, distances=None):
        if not isinstance(table_a, PatchTable) or not isinstance(table_b, PatchTable):
            raise ValueError("PatchOverlaps: table_a and table_b must be PatchTables")
        if table_a.shape != table_b.shape:
            raise ValueError(f"PatchOverlaps: the tables lie on different grids, {table_a.shape} and {table_b.shape}")
        cols = []
        for name, v in (("a", a), ("b", b), ("n", n)):
            v = np.array(v, dtype=np.int64)
            if v.ndim != 1:
                raise ValueError(f"PatchOverlaps: {name} must be one-dimensional, got shape {v.shape}")
            v.setflags(write=False)
            cols.append(v)
        self._a, self._b, self._n = cols
        if not len(self._a) == len(self._b) == len(self._n):
            raise ValueError("PatchOverlaps: a, b and n must have one entry per row")
        if len(self._a) > 1:
            da, db = np.diff(self._a), np.diff(self._b)
            if ((da < 0) | ((da == 0) & (db <= 0))).any():
                raise ValueError("PatchOverlaps: rows must be strictly ascending in (a, b)")
        self.table_a, self.table_b = table_a, table_b
        self._ia = _rows_of(table_a, self._a, "a")
        self._ib = _rows_of(table_b, self._b, "b")
        self._ia.setflags(write=False)
        self._ib.setflags(write=False)
        if ((self._n < 1) | (self._n > np.minimum(table_a.area[self._ia], table_b.area[self._ib]))).any():
            raise ValueError("PatchOverlaps: n must be in 1..min(area_a, area_b)")
        if distances is not None:
            from .proximity import PatchDistances
            if not isinstance(distances, PatchDistances):
                raise ValueError(f"PatchOverlaps: distances must be a PatchDistances or None, got {type(distances).__name__}")
            if distances.table_a != table_a or distances.table_b != table_b:
                raise ValueError("PatchOverlaps: distances need the two PatchTables they belong to")
        self._distances = distances

    a = property(lambda self: self._a)
    b = property(lambda self: self._b)
    n = property(lambda self: self._n)
    inter = property(lambda self: self._n)
    ia = property(lambda self: self._ia)
    ib = property(lambda self: self._ib)
    distances = property(lambda self: self._distances)

    def __len__(self) -> int:
        return len(self._a)

    def union(self) -> np.ndarray:
        """int64 per row: ``area_a + area_b - inter``"""
        return self.table_a.area[self._ia] + self.table_b.area[self._ib] - self._n

    def iou(self) -> np.ndarray:
        """float64 per row: ``inter / union``"""
        return self._n / self.union().astype(np.float64)

    def same_class(self) -> np.ndarray:
        """bool per row: the two patches have the same class"""
        return self.table_a.cls[self._ia] == self.table_b.cls[self._ib]

    def covered_a(self) -> np.ndarray:
        """int64 [n_a]: the pixels of every A patch that some patch of B covers — the sum of ``inter`` over the patch's
        rows, because the patches of one map are disjoint"""
        return _sum_by(self._ia, self._n, self.table_a.n)

    def covered_b(self) -> np.ndarray:
        """int64 [n_b]: ``covered_a`` for the patches of B"""
        return _sum_by(self._ib, self._n, self.table_b.n)

    def _rows(self, same_class: bool) -> np.ndarray:
        return self.same_class() if same_class else np.ones(len(self), bool)

    def partners_a(self, same_class: bool = False) -> np.ndarray:
        """int64 [n_a]: the number of B patches every A patch shares a pixel with (of its own class only with
        ``same_class``)"""
        return np.bincount(self._ia[self._rows(same_class)], minlength=self.table_a.n).astype(np.int64)

    def partners_b(self, same_class: bool = False) -> np.ndarray:
        """int64 [n_b]: ``partners_a`` for the patches of B"""
        return np.bincount(self._ib[self._rows(same_class)], minlength=self.table_b.n).astype(np.int64)

    def __eq__(self, other) -> bool:
        if not isinstance(other, PatchOverlaps):
            return NotImplemented
        if (self._distances is None) != (other._distances is None):
            return False
        return (self.table_a == other.table_a and self.table_b == other.table_b
                and all(np.array_equal(getattr(self, c), getattr(other, c)) for c in ("_a", "_b", "_n"))
                and (self._distances is None or self._distances == other._distances))

    __hash__ = None

    def __repr__(self) -> str:
        tail = "" if self._distances is None else f", distances={self._distances!r}"
        return (f"PatchOverlaps(pairs={len(self)}, n_a={self.table_a.n}, n_b={self.table_b.n}, "
                f"shared pixels={int(self._n.sum())}{tail})")

    # ------------------------------------------------------------------ crown-level accuracy
    def match(self, min_iou: float = 0.5, same_class: bool = True) -> "PatchMatch":
        """one-to-one matching of the patches of A (the reference) and B (the map under test).  Candidates are the rows
        with ``inter * q >= p * union`` in integers, ``p / q = Fraction(min_iou).limit_denominator(10**6)``, of equal
        classes when ``same_class`` is set; they are taken in descending float64 ``iou()``, ties in ascending
        ``(ia, ib)``, and a row is accepted when neither of its patches is taken already.  Above ``min_iou`` 0.5 a patch
        has at most one candidate, so this is THE matching; at or below it is a deterministic greedy one.
        ``0 < min_iou <= 1``"""
        if isinstance(min_iou, bool) or not 0 < min_iou <= 1:
            raise ValueError(f"match: min_iou must satisfy 0 < min_iou <= 1, got {min_iou!r}")
        frac = Fraction(min_iou).limit_denominator(10 ** 6)
        p, q = frac.numerator, frac.denominator
        cand = (self._n * q >= p * self.union()) & self._rows(same_class)
        rows = np.flatnonzero(cand)
        iou = self.iou()
        rows = rows[np.lexsort((self._ib[rows], self._ia[rows], -iou[rows]))]
        a_to_b = np.full(self.table_a.n, -1, np.int64)
        b_to_a = np.full(self.table_b.n, -1, np.int64)
        match_iou = np.full(self.table_a.n, np.nan)
        for r, i, j in zip(rows.tolist(), self._ia[rows].tolist(), self._ib[rows].tolist()):
            if a_to_b[i] < 0 and b_to_a[j] < 0:
                a_to_b[i], b_to_a[j], match_iou[i] = j, i, iou[r]
        return PatchMatch(self.table_a.cls, self.table_b.cls, a_to_b, b_to_a, match_iou)

    # ------------------------------------------------------------------ year-to-year tracks
    def track(self, same_class: bool = False) -> "PatchTracks":
        """the fate of every patch of A (the earlier year) and the origin of every patch of B, from the partner counts
        (``partners_a`` / ``partners_b``; of the patch's own class only with ``same_class``).  ``a_state``: ``VANISHED`` no
        partner; ``SPLIT`` two or more; ``MERGED_INTO`` its single partner has two or more; ``CONTINUED`` exactly one
        partner, which has exactly one (``SPLIT`` goes before ``MERGED_INTO``).  ``b_state``: ``NEW`` no partner;
        ``MERGED`` two or more; ``SPLIT_FROM`` its single partner has two or more; else ``CONTINUED`` (``MERGED`` goes
        before ``SPLIT_FROM``)"""
        rows = self._rows(same_class)
        ia, ib = self._ia[rows], self._ib[rows]
        na, nb = self.table_a.n, self.table_b.n
        pa = np.bincount(ia, minlength=na)
        pb = np.bincount(ib, minlength=nb)
        only_b = np.full(na, -1, np.int64)          # the partner of a patch that has one (any of them otherwise)
        only_b[ia] = ib
        only_a = np.full(nb, -1, np.int64)
        only_a[ib] = ia
        a_state = np.full(na, VANISHED, np.uint8)
        one = pa == 1
        a_state[one] = np.where(pb[only_b[one]] >= 2, MERGED_INTO, CONTINUED)
        a_state[pa >= 2] = SPLIT
        b_state = np.full(nb, NEW, np.uint8)
        one = pb == 1
        b_state[one] = np.where(pa[only_a[one]] >= 2, SPLIT_FROM, CONTINUED)
        b_state[pb >= 2] = MERGED
        growth = np.zeros(nb, np.int64)
        cont = b_state == CONTINUED
        growth[cont] = self.table_b.area[cont] - self.table_a.area[only_a[cont]]
        return PatchTracks(a_state, b_state, growth, self.table_b)


def _sum_by(index: np.ndarray, values: np.ndarray, size: int) -> np.ndarray:
    out = np.zeros(size, np.int64)
    np.add.at(out, index, values)
    return out


def _ratio(num: int, den: int) -> float:
    return num / den if den else float("nan")


class PatchMatch:
    """the result of ``PatchOverlaps.match``: ``a_to_b`` int64 [n_a] (the matched B row, -1 for none), ``b_to_a`` int64
    [n_b]; ``iou`` float64 [n_a] (nan where unmatched); ``tp`` matched pairs, ``fn`` unmatched A patches, ``fp`` unmatched
    B patches; ``recall = tp / n_a``, ``precision = tp / n_b``, ``f1`` (nan on a zero denominator)"""

    def __init__(self, cls_a, cls_b, a_to_b, b_to_a, iou):
        self._cls_a, self._cls_b = cls_a, cls_b
        self.a_to_b, self.b_to_a, self.iou = a_to_b, b_to_a, iou
        for v in (a_to_b, b_to_a, iou):
            v.setflags(write=False)
        self.tp = int(np.count_nonzero(a_to_b >= 0))
        self.fn = len(a_to_b) - self.tp
        self.fp = len(b_to_a) - self.tp

    @property
    def recall(self) -> float:
        return _ratio(self.tp, self.tp + self.fn)

    @property
    def precision(self) -> float:
        return _ratio(self.tp, self.tp + self.fp)

    @property
    def f1(self) -> float:
        return _ratio(2 * self.tp, 2 * self.tp + self.fn + self.fp)

    def per_class(self, K: int) -> np.ndarray:
        """int64 [K - 1, 3]: row ``c - 1`` holds ``tp, fn, fp`` of class ``c`` — a matched pair counts under the class of
        its A patch, an unmatched patch under its own"""
        K = int(K)
        top = max(int(self._cls_a.max()) if len(self._cls_a) else 0, int(self._cls_b.max()) if len(self._cls_b) else 0)
        if not 2 <= K <= MAX_CLASSES or K <= top:
            raise ValueError(f"per_class: K must be in 2..{MAX_CLASSES} and above the largest class {top}, got {K}")
        out = np.zeros((K - 1, 3), np.int64)
        matched = self.a_to_b >= 0
        out[:, 0] = np.bincount(self._cls_a[matched], minlength=K)[1:]
        out[:, 1] = np.bincount(self._cls_a[~matched], minlength=K)[1:]
        out[:, 2] = np.bincount(self._cls_b[self.b_to_a < 0], minlength=K)[1:]
        return out

    def __repr__(self) -> str:
        return (f"PatchMatch(tp={self.tp}, fn={self.fn}, fp={self.fp}, recall={self.recall:.3f}, "
                f"precision={self.precision:.3f}, f1={self.f1:.3f})")


class PatchTracks:
    """the result of ``PatchOverlaps.track``: ``a_state`` uint8 [n_a] (``VANISHED`` 0, ``CONTINUED`` 1, ``SPLIT`` 2,
    ``MERGED_INTO`` 3), ``b_state`` uint8 [n_b] (``NEW`` 0, ``CONTINUED`` 1, ``MERGED`` 2, ``SPLIT_FROM`` 3), ``growth``
    int64 [n_b]: ``area_b - area_a`` of a ``CONTINUED`` patch, 0 otherwise"""

    def __init__(self, a_state, b_state, growth, table_b: PatchTable):
        self.a_state, self.b_state, self.growth = a_state, b_state, growth
        for v in (a_state, b_state, growth):
            v.setflags(write=False)
        self._table_b = table_b

    def counts(self) -> dict:
        """``{"a": {state name: count}, "b": {state name: count}}``"""
        ca = np.bincount(self.a_state, minlength=4)
        cb = np.bincount(self.b_state, minlength=4)
        return {"a": {name: int(ca[k]) for k, name in enumerate(A_STATES)},
                "b": {name: int(cb[k]) for k, name in enumerate(B_STATES)}}

    def new_area_m2(self, pixel_area_m2: Optional[float] = None) -> float:
        """the ground area of the ``NEW`` patches (default pixel size: the B table's)"""
        return float(self._table_b.area_m2(pixel_area_m2)[self.b_state == NEW].sum())

    def __repr__(self) -> str:
        c = self.counts()
        return f"PatchTracks(a={c['a']}, b={c['b']})"


# ---------------------------------------------------------------------------------------------- maps in, table out
def checked_maps(who: str, maps, K: int, configs_in, device=None, shape=None):
    """the maps of ``patch_overlaps`` and its kin where they are read: ``(planes, configs, device)`` — uint8 planes on
    the ``cuda`` device when there is one (device tensors, or ``device`` names one), else host arrays and None; a
    ``PolygonSet`` is burnt with ``all_touched=True``; a configuration None is ``PatchConfig()``.  ``ValueError``: K outside
    2..8, a configuration of a wrong type, a map off the grid, not uint8 or with a value >= K, no grid at all"""
    import torch
    from ..data.polygons import PolygonSet
    from .analysis import check_against_map, map_plane
    K = int(K)
    if not 2 <= K <= MAX_CLASSES:
        raise ValueError(f"{who}: K must be in 2..{MAX_CLASSES}, got {K}")
    configs = []
    for c in configs_in:
        if c is not None and not isinstance(c, PatchConfig):
            raise ValueError(f"{who}: a configuration must be a PatchConfig or None, got {c!r}")
        configs.append(PatchConfig() if c is None else c)
    maps = list(maps)
    dev = None if device is None else torch.device(device)
    for m in maps:
        if isinstance(m, torch.Tensor):
            if shape is None:
                shape = tuple(m.shape)
            if dev is None and m.device.type == "cuda":
                dev = m.device
        elif not isinstance(m, PolygonSet) and shape is None:
            shape = tuple(np.shape(m))
    if shape is None:
        raise ValueError(f"{who}: PolygonSets alone need the grid's shape")
    on_device = dev is not None and dev.type == "cuda"
    for k, m in enumerate(maps):
        if isinstance(m, torch.Tensor):
            if m.dtype != torch.uint8 or tuple(m.shape) != tuple(shape) or m.dim() != 2 or m.numel() == 0:
                raise ValueError(f"{who}: a map must be uint8 on the grid {tuple(shape)}, got {m.dtype} "
                                 f"{tuple(m.shape)}")
            maps[k] = m.to(dev) if on_device else check_against_map(m.cpu().numpy(), shape, K, who)
            continue
        maps[k] = map_plane(check_against_map(m, shape, K, who), shape, True, dev if on_device else None)
    return maps, configs, dev if on_device else None


def labelled_maps(who: str, maps, K: int, configs, device=None, shape=None):
    """label -> (sieve) -> table of every map of ``checked_maps``: ``(label planes, PatchTables, device)`` — on the host
    (``device`` None) ``labelled_patches_host``, on a ``cuda`` device ``analysis.device_patches``: the label planes stay
    there and only the tables are downloaded.  No input is written"""
    maps, configs, dev = checked_maps(who, maps, K, configs, device, shape)
    K = int(K)
    if dev is None:
        planes = [labelled_patches_host(m, K, c) for m, c in zip(maps, configs)]
        return [p[1] for p in planes], [p[2] for p in planes], None
    import torch
    from .analysis import device_patches
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    planes = [device_patches(m, K, c, err) for m, c in zip(maps, configs)]
    if int(err.cpu()):
        raise ValueError(f"{who}: class value out of range (K={K})")
    return [p[0] for p in planes], [p[1] for p in planes], dev


def patch_overlaps(map_a, map_b, K: int, config_a: Optional[PatchConfig] = None, config_b: Optional[PatchConfig] = None,
                   device=None, shape=None) -> PatchOverlaps:
    """the ``PatchOverlaps`` of two maps on one grid: uint8 class maps (arrays or tensors), or ``PolygonSet``s in pixel
    coordinates, burnt with ``rasterize(..., all_touched=True)`` — the rule the training masks are made with; a polygon
    value >= K is a ``ValueError``.  Label -> (sieve) -> table on both maps (``config_a`` / ``config_b``, default
    ``PatchConfig()``), then the overlap table.  ``shape``: the grid, needed only when both maps are polygons.

    On the host ``labelled_patches_host`` + ``overlap_pairs_host``.  With device tensors, or ``device`` a ``cuda`` device,
    ``ops.label_patches`` -> ``ops.patch_areas`` -> (``ops.sieve_patches``) -> ``ops.patch_table`` on both maps, then
    ``ops.patch_overlaps``: only the tables are downloaded.  Neither input is written"""
    (labels_a, labels_b), (table_a, table_b), dev = labelled_maps("patch_overlaps", (map_a, map_b), K, (config_a, config_b),
                                                                  device, shape)
    if dev is None:
        return PatchOverlaps(table_a, table_b, *overlap_pairs_host(labels_a, labels_b))
    from .. import ops
    return PatchOverlaps(table_a, table_b, *ops.patch_overlaps(labels_a, labels_b))
