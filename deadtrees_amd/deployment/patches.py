"""Dead-tree patches: the connected components of a predicted class map — how many dead crowns or stands a raster holds,
how large they are and where, and the map without the one- and two-pixel speckle of an arg-max (a minimum mapping unit,
applied before the map is vectorised against the reference's polygon ground truth, the ``deadtrees_20xx`` shapefiles).

The contract, in one place (the device path, ``csrc/patches.hip`` through ``ops.label_patches`` / ``ops.patch_areas`` /
``ops.sieve_patches`` / ``ops.patch_table``, computes exactly this; the functions below are the CPU path and the tests'
oracle):

* a **patch** is a maximal set of pixels of the SAME class ``c``, ``1 <= c < K``, connected through 4-neighbourhoods
  (``connectivity=4``) or 8-neighbourhoods (``connectivity=8``, the default).  Class 0 is background and is never
  labelled; pixels of class 1 and class 2 that touch are two patches;
* **labels** int32 ``[h, w]``: 0 on background, elsewhere ``1 + min(y * w + x)`` over the pixels of the pixel's patch — a
  label names its patch's first pixel in row-major order.  The plane is therefore unique: it depends on no launch order,
  batch size or implementation, and device and host compare with ``array_equal``.  ``h * w <= 2**31 - 2``;
* the **table** (``PatchTable``) has one row per patch in ascending ``root``; integers only, centroids are exact
  rationals ``sum / area``;
* the **sieve** turns every patch smaller than ``min_pixels`` into background and changes nothing else.

numpy only; ``scipy.ndimage`` is imported lazily by ``label_patches_host`` (as ``data/distmap.py`` does).
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

from .stats import MAX_CLASSES, PIXEL_AREA_M2

MAX_PIXELS = 2 ** 31 - 2      # labels are int32 and 1-based


class PatchConfig:
    """what ``infer_tile(..., stats=True, patches=...)`` is asked for: ``connectivity`` 4 or 8, ``min_pixels`` >= 0 — patches
    with fewer pixels are sieved out of the returned map (``min_pixels <= 1``: no sieve)"""

    def __init__(self, connectivity: int = 8, min_pixels: int = 0):
        if isinstance(connectivity, bool) or connectivity not in (4, 8):
            raise ValueError(f"PatchConfig: connectivity must be 4 or 8, got {connectivity!r}")
        if isinstance(min_pixels, bool) or int(min_pixels) != min_pixels or min_pixels < 0:
            raise ValueError(f"PatchConfig: min_pixels must be an integer >= 0, got {min_pixels!r}")
        self.connectivity = int(connectivity)
        self.min_pixels = int(min_pixels)

    @property
    def sieves(self) -> bool:
        return self.min_pixels > 1

    def __eq__(self, other) -> bool:
        if not isinstance(other, PatchConfig):
            return NotImplemented
        return (self.connectivity, self.min_pixels) == (other.connectivity, other.min_pixels)

    __hash__ = None

    def __repr__(self) -> str:
        return f"PatchConfig(connectivity={self.connectivity}, min_pixels={self.min_pixels})"


def check_patches(patches) -> Optional[PatchConfig]:
    """the ``patches`` argument of ``infer_tile`` / ``Tiler.stats`` -> ``PatchConfig`` or None (None / False: not asked
    for; True: the defaults); anything else is a ``ValueError``"""
    if patches is None or patches is False:
        return None
    if patches is True:
        return PatchConfig()
    if isinstance(patches, PatchConfig):
        return patches
    raise ValueError(f"patches must be True, False, None or a PatchConfig, got {patches!r}")


def _check_map(classes, what: str) -> np.ndarray:
    c = np.asarray(classes)
    if c.dtype != np.uint8:
        raise ValueError(f"{what}: classes must be uint8, got {c.dtype}")
    if c.ndim != 2 or c.size == 0:
        raise ValueError(f"{what}: classes must be a non-empty [h, w] map, got shape {c.shape}")
    if c.size > MAX_PIXELS:
        raise ValueError(f"{what}: {c.size} pixels do not fit int32 labels (h * w <= {MAX_PIXELS})")
    return c


def _check_labels(labels, shape, what: str) -> np.ndarray:
    lab = np.asarray(labels)
    if lab.dtype != np.int32:
        raise ValueError(f"{what}: labels must be int32, got {lab.dtype}")
    if tuple(lab.shape) != tuple(shape):
        raise ValueError(f"{what}: labels {tuple(lab.shape)} and classes {tuple(shape)} must have the same shape")
    return lab


def label_patches_host(classes_u8, K: int, connectivity: int = 8) -> np.ndarray:
    """int32 [h, w] labels of the module's contract: 0 on class 0, elsewhere 1 + the row-major index of the first pixel of
    the pixel's patch.  2 <= K <= 8; a class value >= K is a ``ValueError`` (the device ORs 1 into its ``err`` flag and
    treats the pixel as background)"""
    from scipy import ndimage
    K = int(K)
    if not 2 <= K <= MAX_CLASSES:
        raise ValueError(f"label_patches: K must be in 2..{MAX_CLASSES}, got {K}")
    if connectivity not in (4, 8):
        raise ValueError(f"label_patches: connectivity must be 4 or 8, got {connectivity!r}")
    c = _check_map(classes_u8, "label_patches")
    if int(c.max()) >= K:
        raise ValueError(f"label_patches: class value {int(c.max())} out of range (K={K})")
    structure = np.ones((3, 3), bool) if connectivity == 8 else ndimage.generate_binary_structure(2, 1)
    labels = np.zeros(c.size, np.int32)
    for cls in range(1, K):
        comp, n = ndimage.label(c == cls, structure=structure)
        if n == 0:
            continue
        comp = comp.ravel()
        at = np.flatnonzero(comp)                                  # ascending: the first hit of a component is its minimum
        ids, first = np.unique(comp[at], return_index=True)
        root = np.zeros(n + 1, np.int64)
        root[ids] = at[first]
        labels[at] = (root[comp[at]] + 1).astype(np.int32)
    return labels.reshape(c.shape)


class PatchTable:
    """one row per patch, in ascending ``root``; numpy only and read-only, like ``RasterStats``.  ``root`` int64: row-major
    index of the patch's first pixel (its label minus 1); ``cls`` uint8; ``area`` int64, pixels; ``bbox`` int32 [n, 4]:
    ``y0, x0, y1, x1``, inclusive; ``sum_y`` / ``sum_x`` int64: the sums of the pixels' row / column numbers, so that the
    centroid ``sum / area`` is an exact rational.  ``shape`` is the (h, w) of the raster the roots index into"""

    _FIELDS = (("root", np.int64, 1), ("cls", np.uint8, 1), ("area", np.int64, 1), ("bbox", np.int32, 2),
               ("sum_y", np.int64, 1), ("sum_x", np.int64, 1))

    def __init__(self, root, cls, area, bbox, sum_y, sum_x, shape: Tuple[int, int],
                 pixel_area_m2: float = PIXEL_AREA_M2):
        given = dict(root=root, cls=cls, area=area, bbox=bbox, sum_y=sum_y, sum_x=sum_x)
        n = len(np.asarray(root))
        for name, dtype, ndim in self._FIELDS:
            a = np.array(given[name], dtype=dtype)
            if ndim == 2:
                a = a.reshape(-1, 4)
            if a.ndim != ndim or len(a) != n:
                raise ValueError(f"PatchTable: {name} must hold one row per patch ({n}), got shape {a.shape}")
            a.setflags(write=False)
            setattr(self, "_" + name, a)
        if n and ((np.diff(self._root) <= 0).any() or self._root[0] < 0):
            raise ValueError("PatchTable: roots must be ascending and >= 0")
        self.shape = (int(shape[0]), int(shape[1]))
        self.pixel_area_m2 = float(pixel_area_m2)

    root = property(lambda self: self._root)
    cls = property(lambda self: self._cls)
    area = property(lambda self: self._area)
    bbox = property(lambda self: self._bbox)
    sum_y = property(lambda self: self._sum_y)
    sum_x = property(lambda self: self._sum_x)

    @property
    def n(self) -> int:
        return len(self._root)

    def __len__(self) -> int:
        return self.n

    def count(self, cls: Optional[int] = None) -> int:
        """the number of patches, of class ``cls`` when one is given"""
        return self.n if cls is None else int(np.count_nonzero(self._cls == cls))

    def centroids(self) -> np.ndarray:
        """float64 [n, 2]: (y, x) = (sum_y / area, sum_x / area), pixel centres at integer coordinates"""
        area = self._area.astype(np.float64)
        return np.stack([self._sum_y / area, self._sum_x / area], axis=1) if self.n else np.zeros((0, 2))

    def area_m2(self, pixel_area_m2: Optional[float] = None) -> np.ndarray:
        """float64 [n]: ``area`` times the ground size of a pixel (default: the table's, ``PIXEL_AREA_M2``)"""
        return self._area * (self.pixel_area_m2 if pixel_area_m2 is None else float(pixel_area_m2))

    def size_histogram(self, edges, K: Optional[int] = None) -> np.ndarray:
        """int64 [K - 1, len(edges) + 1]: row ``c - 1`` counts the patches of class ``c`` by area in pixels.  ``edges`` is
        ascending; bin 0 holds ``area < edges[0]``, bin ``j`` holds ``edges[j - 1] <= area < edges[j]`` and the last bin
        ``area >= edges[-1]`` (``np.searchsorted(edges, area, side="right")``).  ``K`` defaults to ``max(2, cls.max() +
        1)``"""
        edges = np.asarray(edges)
        if edges.ndim != 1 or len(edges) == 0 or (np.diff(edges) <= 0).any():
            raise ValueError("size_histogram: edges must be a non-empty ascending sequence")
        top = int(self._cls.max()) + 1 if self.n else 2
        K = max(2, top) if K is None else int(K)
        if K < top:
            raise ValueError(f"size_histogram: K={K} is smaller than the table's largest class + 1 = {top}")
        hist = np.zeros((K - 1, len(edges) + 1), np.int64)
        np.add.at(hist, (self._cls.astype(np.intp) - 1, np.searchsorted(edges, self._area, side="right")), 1)
        return hist

    def __eq__(self, other) -> bool:
        if not isinstance(other, PatchTable):
            return NotImplemented
        return (self.shape == other.shape and self.pixel_area_m2 == other.pixel_area_m2
                and all(np.array_equal(getattr(self, "_" + name), getattr(other, "_" + name))
                        for name, _, _ in self._FIELDS))

    __hash__ = None

    def __repr__(self) -> str:
        return (f"PatchTable(n={self.n}, shape={self.shape}, per class={np.bincount(self._cls, minlength=2)[1:].tolist()}, "
                f"pixels={int(self._area.sum())})")


def measure_patches_host(labels, classes_u8) -> PatchTable:
    """the table of a label plane (``label_patches_host``, sieved or not) and its class map.  ``ValueError`` when the two
    do not belong together: a label on background or none on a class, or a label that names no pixel of the map"""
    c = _check_map(classes_u8, "measure_patches")
    lab = _check_labels(labels, c.shape, "measure_patches")
    h, w = c.shape
    if ((lab != 0) != (c != 0)).any() or int(lab.min()) < 0 or int(lab.max()) > c.size:
        raise ValueError("measure_patches: labels and classes do not belong together")
    flat = lab.ravel()
    at = np.flatnonzero(flat)
    root, row = np.unique(flat[at].astype(np.int64) - 1, return_inverse=True)
    n = len(root)
    if n and not np.array_equal(flat[root], root + 1):
        raise ValueError("measure_patches: a label does not name its patch's first pixel")
    y, x = at // w, at % w
    bbox = np.empty((n, 4), np.int32)
    for col, (v, op, start) in enumerate(((y, np.minimum, h), (x, np.minimum, w), (y, np.maximum, -1),
                                          (x, np.maximum, -1))):
        ext = np.full(n, start, np.int64)
        op.at(ext, row, v)
        bbox[:, col] = ext
    sum_y, sum_x = np.zeros(n, np.int64), np.zeros(n, np.int64)
    np.add.at(sum_y, row, y)
    np.add.at(sum_x, row, x)
    return PatchTable(root, c.ravel()[root], np.bincount(row, minlength=n), bbox, sum_y, sum_x, (h, w))


def sieve_host(classes_u8, labels, min_pixels: int):
    """(classes', labels'): every patch with ``area < min_pixels`` becomes class 0 / label 0; nothing else changes, and
    ``min_pixels <= 1`` changes nothing at all.  A removed patch is NOT filled from its neighbours as ``gdal_sieve`` does:
    it becomes background.  Removing patches never merges or splits the remaining ones, so the labels of the survivors
    stay valid (``labels'`` is the label plane of ``classes'``).  Both results are new arrays"""
    c = _check_map(classes_u8, "sieve")
    lab = _check_labels(labels, c.shape, "sieve")
    if isinstance(min_pixels, bool) or int(min_pixels) != min_pixels or min_pixels < 0:
        raise ValueError(f"sieve: min_pixels must be an integer >= 0, got {min_pixels!r}")
    c, lab = c.copy(), lab.copy()
    if min_pixels > 1:
        area = np.bincount(lab.ravel(), minlength=1)
        small = area[lab] < min_pixels
        small &= lab != 0
        c[small] = 0
        lab[small] = 0
    return c, lab


def labelled_patches_host(classes_u8, K: int, config: PatchConfig, crowns=None):
    """label -> sieve -> measure on the host: (classes', labels', PatchTable); ``classes'`` is ``classes_u8`` itself when
    the configuration does not sieve, ``labels'`` the label plane of ``classes'``.  With ``crowns`` (a ``CrownConfig``,
    ``deployment/crowns.py``) the patches are split behind the sieve: ``labels'`` is the crown plane, the table has one row per
    crown, and a fourth item is the ``CrownSplit``"""
    c = np.ascontiguousarray(classes_u8)
    labels = label_patches_host(c, K, config.connectivity)
    if config.sieves:
        c, labels = sieve_host(c, labels, config.min_pixels)
    if crowns is not None:
        from .crowns import crowned_patches_host
        return (c,) + crowned_patches_host(c, labels, K, config.connectivity, crowns)
    return c, labels, measure_patches_host(labels, c)


def patches_host(classes_u8, K: int, config: PatchConfig):
    """``labelled_patches_host`` without the label plane: (classes', PatchTable) — what the host paths of ``infer_tile``
    and ``Tiler.stats`` run"""
    c, _, table = labelled_patches_host(classes_u8, K, config)
    return c, table
