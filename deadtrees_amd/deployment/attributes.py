"""Patch attributes: what every dead-tree patch looks like in the raster it was found in — band means, spread and
extremes, normalised differences such as NDVI — and how sure the model was of it: mean and minimum class probability.
``PatchTable`` says where a patch is and how large; this says which detections are weak and what their spectra are.

The contract, in one place (the device path, ``csrc/attributes.hip`` through ``ops.patch_attributes``, computes
exactly this; ``patch_attributes_host`` is the CPU path).  Everything is an integer, so device and host compare with
``array_equal``:

* ``L`` is a label plane of ``deployment/patches.py``: int32 ``[h, w]``, 0 on background, elsewhere ``1 + root``; the raster is
  uint8 ``[C, h, w]`` on the same grid, ``1 <= C <= 8``.  Row ``r`` of a ``PatchTable`` takes the pixels with
  ``L == 1 + root[r]``;
* per band ``c``: ``band_sum[r, c]`` and ``band_sumsq[r, c]`` int64, ``band_min[r, c]`` and ``band_max[r, c]`` uint8;
* per index pair ``(a, b)``, at most 4: a pixel has ``s = v_a + v_b`` and ``t = (v_a * 65534 + (s >> 1)) // s``, unsigned —
  ``round(65534 * v_a / s)`` in ``[0, 65534]``, and 32767 for ``s == 0``.  ``index_sum[r, k]`` is the int64 sum of ``t``; the
  normalised difference ``(v_a - v_b) / (v_a + v_b)`` of the pixel is ``(t - 32767) / 32767``.  The default pair is
  ``(3, 0)`` — NDVI in the reference's RGBN band order — when ``C >= 4``, none otherwise;
* confidence, only with the fp32 probabilities ``[K, h, w]`` and the class map: for ``p = probs[map[i], i]`` take
  ``p' = p if p > 0 else 0`` (NaN becomes 0), ``p' = min(p', 1)`` and ``q = floor(p' * 65535 + 0.5)``, the product and the sum
  each rounded to float32 (``np.float32`` arithmetic here, ``-ffp-contract=off`` there).  ``conf_sum[r]`` int64 is the sum of
  ``q``, ``conf_min[r]`` its minimum, in ``[0, 65535]``;
* a root without a pixel in ``L`` has sums 0, minima 255 (65535 for ``conf_min``) and maxima 0;
* sides <= 16384 and ``h * w <= 2**31 - 2``.

numpy and the standard library only.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

from .patches import MAX_PIXELS, PatchConfig, PatchTable
from .stats import MAX_CLASSES

MAX_SIDE = 16384
MAX_BANDS = 8
MAX_INDICES = 4
T_SCALE = 65534                  # t of a pixel with v_b == 0
T_ZERO = 32767                   # t of a pixel with v_a == v_b, and of one with v_a + v_b == 0
Q_SCALE = 65535                  # q of probability 1
NDVI = (3, 0)                    # (NIR, red) of an RGBN raster


def index_t(v_a, v_b) -> np.ndarray:
    """int64: the quantised share ``v_a / (v_a + v_b)`` of the contract, elementwise over uint8 values"""
    a, b = np.asarray(v_a).astype(np.int64), np.asarray(v_b).astype(np.int64)
    s = a + b
    return np.where(s > 0, (a * T_SCALE + (s >> 1)) // np.maximum(s, 1), T_ZERO)


def confidence_q(p) -> np.ndarray:
    """int64: the quantised probability of the contract, elementwise over float32 values"""
    p = np.asarray(p, dtype=np.float32)
    p = np.minimum(np.where(p > 0, p, np.float32(0)), np.float32(1))
    return np.floor(p * np.float32(Q_SCALE) + np.float32(0.5)).astype(np.int64)


def _pair(item):
    try:
        a, b = item
    except (TypeError, ValueError):
        raise ValueError(f"AttributeConfig: index {item!r}: expected a pair of band numbers") from None
    for v in (a, b):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v < MAX_BANDS:
            raise ValueError(f"AttributeConfig: index {item!r}: band numbers are integers in 0..{MAX_BANDS - 1}")
    return int(a), int(b)


class AttributeConfig:
    """what ``attributes=`` is asked for: ``indices``, up to 4 band pairs ``(a, b)`` whose normalised difference
    ``(v_a - v_b) / (v_a + v_b)`` is averaged per patch (None: NDVI ``(3, 0)`` for a raster of four bands or more, nothing
    for a smaller one), and ``confidence``: the mean and minimum probability of the patch's class as well, where the call
    has probabilities"""

    def __init__(self, indices=None, confidence: bool = False):
        if not isinstance(confidence, (bool, np.bool_)):
            raise ValueError(f"AttributeConfig: confidence must be True or False, got {confidence!r}")
        if indices is not None:
            try:
                indices = tuple(_pair(item) for item in indices)
            except TypeError:
                raise ValueError(f"AttributeConfig: indices must be a sequence of band pairs or None, got {indices!r}") from None
            if len(indices) > MAX_INDICES:
                raise ValueError(f"AttributeConfig: at most {MAX_INDICES} index pairs, got {len(indices)}")
        self.indices = indices
        self.confidence = bool(confidence)

    def pairs(self, C: int) -> Tuple[Tuple[int, int], ...]:
        """the index pairs for a raster of ``C`` bands; a band number >= C is a ``ValueError``"""
        if self.indices is None:
            return (NDVI,) if C >= 4 else ()
        for a, b in self.indices:
            if max(a, b) >= C:
                raise ValueError(f"attributes: index ({a}, {b}) names a band the {C}-band raster does not have")
        return self.indices

    def __eq__(self, other) -> bool:
        if not isinstance(other, AttributeConfig):
            return NotImplemented
        return (self.indices, self.confidence) == (other.indices, other.confidence)

    __hash__ = None

    def __repr__(self) -> str:
        return f"AttributeConfig(indices={self.indices!r}, confidence={self.confidence})"


def check_attributes(option) -> Optional[AttributeConfig]:
    """the ``attributes`` argument of ``infer_tile`` -> ``AttributeConfig`` or None (None / False: not asked for; True: the
    defaults); anything else is a ``ValueError``"""
    if option is None or option is False:
        return None
    if option is True:
        return AttributeConfig()
    if isinstance(option, AttributeConfig):
        return option
    raise ValueError(f"attributes must be True, False, None or an AttributeConfig, got {option!r}")


def check_raster(raster, shape=None, what: str = "patch_attributes"):
    """the raster's band count after its checks: uint8 ``[C, h, w]`` (anything with ``dtype`` and ``shape``), ``1 <= C <= 8``,
    on the grid ``shape`` when one is given, sides <= 16384 and ``h * w <= 2**31 - 2``; ``ValueError`` otherwise"""
    dtype, dims = getattr(raster, "dtype", None), tuple(getattr(raster, "shape", ()))
    if dtype is None or str(dtype).replace("torch.", "") != "uint8":
        raise ValueError(f"{what}: the raster must be uint8, got {dtype}")
    if len(dims) != 3 or not 1 <= dims[0] <= MAX_BANDS:
        raise ValueError(f"{what}: the raster must be [C, h, w] with 1 <= C <= {MAX_BANDS}, got shape {dims}")
    if shape is not None and dims[1:] != tuple(shape):
        raise ValueError(f"{what}: the raster {dims[1:]} must lie on the map's grid {tuple(shape)}")
    h, w = dims[1:]
    if min(h, w) < 1 or max(h, w) > MAX_SIDE or h * w > MAX_PIXELS:
        raise ValueError(f"{what}: a raster of {(h, w)}: sides must be in 1..{MAX_SIDE}, h * w <= {MAX_PIXELS}")
    return int(dims[0])


def table_columns(C: int, n_pairs: int, confidence: bool) -> Tuple[int, int]:
    """``(Q, M)``: the columns of the two tables both paths fill.  Sums: band sums ``[0, C)``, sums of squares ``[C, 2C)``, index
    sums ``[2C, 2C + I)``, then the confidence sum; extremes: band minima ``[0, C)``, maxima ``[C, 2C)``, then the confidence
    minimum"""
    return 2 * C + n_pairs + (1 if confidence else 0), 2 * C + (1 if confidence else 0)


def attribute_tables_host(labels, roots, raster, classes=None, probs=None, indices=()):
    """the module's contract in numpy: ``(sums int64 [n, Q], extremes int32 [n, M])`` in the layout of ``table_columns``, one
    row per element of ``roots`` (ascending).  ``ValueError``: labels that are not int32 ``[h, w]``, a raster of ``check_raster``,
    a band number >= C, probabilities that are not float32 ``[K, h, w]`` or come without a uint8 class map, a class >= K"""
    lab = np.asarray(labels)
    if lab.dtype != np.int32 or lab.ndim != 2:
        raise ValueError(f"patch_attributes: labels must be int32 [h, w], got {lab.dtype} {lab.shape}")
    raster = np.asarray(raster)
    C = check_raster(raster, lab.shape)
    pairs = AttributeConfig(indices).pairs(C)
    if (classes is None) != (probs is None):
        raise ValueError("patch_attributes: probabilities come with their class map, and the other way round")
    roots = np.asarray(roots).astype(np.int64).ravel()
    n = len(roots)
    Q, M = table_columns(C, len(pairs), probs is not None)
    sums, ext = np.zeros((n, Q), np.int64), np.zeros((n, M), np.int32)
    ext[:, :C] = 255
    flat = lab.ravel()
    at = np.flatnonzero(flat > 0)
    row = np.searchsorted(roots, flat[at].astype(np.int64) - 1)
    known = (row < n) & (roots[np.minimum(row, max(n - 1, 0))] == flat[at] - 1) if n else np.zeros(len(at), bool)
    at, row = at[known], row[known]
    bands = raster.reshape(C, -1)[:, at].astype(np.int64)
    for c in range(C):
        np.add.at(sums[:, c], row, bands[c])
        np.add.at(sums[:, C + c], row, bands[c] * bands[c])
        np.minimum.at(ext[:, c], row, bands[c])
        np.maximum.at(ext[:, C + c], row, bands[c])
    for k, (a, b) in enumerate(pairs):
        np.add.at(sums[:, 2 * C + k], row, index_t(bands[a], bands[b]))
    if probs is not None:
        probs, classes = np.asarray(probs), np.asarray(classes)
        if probs.dtype != np.float32 or probs.ndim != 3 or probs.shape[1:] != lab.shape or not 2 <= len(probs) <= MAX_CLASSES:
            raise ValueError(f"patch_attributes: probabilities must be float32 [K, h, w] on the map's grid with 2 <= K <= "
                             f"{MAX_CLASSES}, got {probs.dtype} {probs.shape}")
        if classes.dtype != np.uint8 or classes.shape != lab.shape:
            raise ValueError(f"patch_attributes: the class map must be uint8 {lab.shape}, got {classes.dtype} {classes.shape}")
        cls = classes.ravel()[at]
        if len(cls) and int(cls.max()) >= len(probs):
            raise ValueError(f"patch_attributes: class value {int(cls.max())} out of range (K={len(probs)})")
        q = confidence_q(probs.reshape(len(probs), -1)[cls, at])
        ext[:, 2 * C] = Q_SCALE
        np.add.at(sums[:, Q - 1], row, q)
        np.minimum.at(ext[:, 2 * C], row, q)
    return sums, ext


def _read_only(a, dtype) -> np.ndarray:
    a = np.array(a, dtype=dtype)
    a.setflags(write=False)
    return a


class PatchAttributes:
    """the attributes of the patches of ONE map, aligned with its ``PatchTable``; numpy only and read-only.  ``bands``: C;
    ``indices``: the band pairs; ``band_sum`` / ``band_sumsq`` int64 [n, C], ``band_min`` / ``band_max`` uint8 [n, C],
    ``index_sum`` int64 [n, I], ``conf_sum`` int64 [n] and ``conf_min`` int32 [n] (both None without confidence): the
    integers of the module's contract.  The floats are read off them in float64"""

    def __init__(self, table: PatchTable, sums, extremes, bands: int, indices=(), confidence: bool = False):
        if not isinstance(table, PatchTable):
            raise ValueError("PatchAttributes: table must be a PatchTable")
        self.table, self.bands, self.indices = table, int(bands), tuple((int(a), int(b)) for a, b in indices)
        C, I = self.bands, len(self.indices)
        Q, M = table_columns(C, I, confidence)
        sums, extremes = np.asarray(sums), np.asarray(extremes)
        if sums.shape != (table.n, Q) or extremes.shape != (table.n, M):
            raise ValueError(f"PatchAttributes: expected tables of {(table.n, Q)} and {(table.n, M)}, got {sums.shape} and "
                             f"{extremes.shape}")
        self._band_sum, self._band_sumsq = _read_only(sums[:, :C], np.int64), _read_only(sums[:, C:2 * C], np.int64)
        self._index_sum = _read_only(sums[:, 2 * C:2 * C + I], np.int64)
        self._band_min, self._band_max = _read_only(extremes[:, :C], np.uint8), _read_only(extremes[:, C:2 * C], np.uint8)
        self._conf_sum = _read_only(sums[:, Q - 1], np.int64) if confidence else None
        self._conf_min = _read_only(extremes[:, 2 * C], np.int32) if confidence else None

    band_sum = property(lambda self: self._band_sum)
    band_sumsq = property(lambda self: self._band_sumsq)
    band_min = property(lambda self: self._band_min)
    band_max = property(lambda self: self._band_max)
    index_sum = property(lambda self: self._index_sum)
    conf_sum = property(lambda self: self._conf_sum)
    conf_min = property(lambda self: self._conf_min)

    @property
    def has_confidence(self) -> bool:
        return self._conf_sum is not None

    def _area(self) -> np.ndarray:
        return self.table.area.astype(np.float64)

    def mean(self) -> np.ndarray:
        """float64 [n, C]: the band means"""
        return self._band_sum / self._area()[:, None]

    def std(self) -> np.ndarray:
        """float64 [n, C]: the population standard deviation, from sum and sum of squares"""
        area = self._area()[:, None]
        mean = self._band_sum / area
        return np.sqrt(np.maximum(self._band_sumsq / area - mean * mean, 0.0))

    def index(self, k: int = 0) -> np.ndarray:
        """float64 [n]: the patch mean of the normalised difference of pair ``k``, in [-1, 1]"""
        if not 0 <= k < len(self.indices):
            raise ValueError(f"PatchAttributes: index {k} of {len(self.indices)} pairs")
        return (self._index_sum[:, k] / self._area() - T_ZERO) / T_ZERO

    def _need_confidence(self):
        if self._conf_sum is None:
            raise ValueError("PatchAttributes: computed without confidence (AttributeConfig(confidence=True))")

    def confidence(self) -> np.ndarray:
        """float64 [n]: the mean probability of the patch's class over its pixels, in [0, 1]"""
        self._need_confidence()
        return self._conf_sum / self._area() / Q_SCALE

    def min_confidence(self) -> np.ndarray:
        """float64 [n]: the smallest probability of the patch's class among its pixels, in [0, 1]"""
        self._need_confidence()
        return self._conf_min / float(Q_SCALE)

    def index_name(self, k: int) -> str:
        """the ``properties`` column of pair ``k``: ``ndvi`` for (3, 0), else ``nd_<a>_<b>``"""
        a, b = self.indices[k]
        return "ndvi" if (a, b) == NDVI else f"nd_{a}_{b}"

    def properties(self, names=None) -> dict:
        """``{column: one entry per patch}`` for ``outlines_geojson(..., properties=...)``: ``mean_b<c>``, ``std_b<c>``,
        ``min_b<c>``, ``max_b<c>`` per band, ``ndvi`` / ``nd_<a>_<b>`` per pair, ``confidence`` and ``min_confidence`` when there
        are any.  ``names``: the columns wanted, in that order (None: all); an unknown one is a ``ValueError``"""
        mean, std = self.mean(), self.std()
        columns = {}
        for c in range(self.bands):
            columns[f"mean_b{c}"], columns[f"std_b{c}"] = mean[:, c], std[:, c]
            columns[f"min_b{c}"], columns[f"max_b{c}"] = self._band_min[:, c], self._band_max[:, c]
        for k in range(len(self.indices)):
            columns[self.index_name(k)] = self.index(k)
        if self.has_confidence:
            columns["confidence"], columns["min_confidence"] = self.confidence(), self.min_confidence()
        if names is None:
            return columns
        unknown = [name for name in names if name not in columns]
        if unknown:
            raise ValueError(f"PatchAttributes: no column {unknown[0]!r} (there are {', '.join(columns)})")
        return {name: columns[name] for name in names}

    _ARRAYS = ("_band_sum", "_band_sumsq", "_band_min", "_band_max", "_index_sum", "_conf_sum", "_conf_min")

    def __eq__(self, other) -> bool:
        if not isinstance(other, PatchAttributes):
            return NotImplemented
        return (self.table == other.table and self.bands == other.bands and self.indices == other.indices
                and self.has_confidence == other.has_confidence
                and all(np.array_equal(getattr(self, a), getattr(other, a)) for a in self._ARRAYS
                        if getattr(self, a) is not None))

    __hash__ = None

    def __repr__(self) -> str:
        tail = ""
        if self.has_confidence and self.table.n:
            tail = f", weakest mean confidence {float(self.confidence().min()):.3f}"
        return (f"PatchAttributes(n={self.table.n}, bands={self.bands}, indices={list(self.indices)}, "
                f"confidence={self.has_confidence}{tail})")


# ---------------------------------------------------------------------------------------------- label planes in
def attributes_of(labels, table: PatchTable, raster, classes=None, probs=None, config: Optional[AttributeConfig] = None,
                  device: bool = False) -> PatchAttributes:
    """``PatchAttributes`` of a label plane, its table and a raster on its grid under ``config`` (None: the defaults):
    through ``ops.patch_attributes`` with ``device`` (everything but the table is a device tensor), else
    ``attribute_tables_host``.  ``classes`` and ``probs`` are read only with ``config.confidence``, and then both are needed"""
    config = AttributeConfig() if config is None else config
    pairs = config.pairs(check_raster(raster, tuple(table.shape)))
    if config.confidence and (classes is None or probs is None):
        raise ValueError("patch_attributes: confidence needs the class map and its probabilities")
    if not config.confidence:
        classes = probs = None
    if device:
        from ..ops import patch_attributes as run
    else:
        run = attribute_tables_host
    sums, extremes = run(labels, table.root, raster, classes, probs, pairs)
    return PatchAttributes(table, sums, extremes, raster.shape[0], pairs, config.confidence)


def patch_attributes_host(labels, table: PatchTable, raster, classes=None, probs=None,
                          config: Optional[AttributeConfig] = None) -> PatchAttributes:
    """the ``PatchAttributes`` of a host label plane (``label_patches_host``, sieved or not) and its ``PatchTable`` in numpy.
    ``config`` None: the default indices, and confidence when ``probs`` are given"""
    if config is None:
        config = AttributeConfig(confidence=probs is not None)
    return attributes_of(labels, table, np.asarray(raster), classes, probs, config)


# ---------------------------------------------------------------------------------------------- maps in
def patch_attributes(map, raster, K: int, probs=None, patches: Optional[PatchConfig] = None,
                     config: Optional[AttributeConfig] = None, device=None) -> PatchAttributes:
    """the ``PatchAttributes`` of one map over a raster on its grid.  ``map`` is taken as ``overlaps.patch_overlaps`` takes its
    maps: a uint8 class map (array or tensor) or a ``PolygonSet`` in pixel coordinates (burnt with ``all_touched=True``), so
    that the spectra of annotated crowns come from the same call; label -> (sieve) -> table under ``patches`` (default
    ``PatchConfig()``), then the attributes under ``config`` (None: the default indices, confidence when ``probs`` are given).
    ``raster`` uint8 ``[C, h, w]`` and ``probs`` float32 ``[K, h, w]``: arrays or tensors.  On the host
    ``patch_attributes_host``; with a device tensor for the map, or ``device`` a ``cuda`` device, ``ops.patch_attributes`` on the
    planes in HBM: only the two tables are downloaded.  No input is written"""
    from .overlaps import checked_maps, labelled_maps
    if config is None:
        config = AttributeConfig(confidence=probs is not None)
    elif not isinstance(config, AttributeConfig):
        raise ValueError(f"patch_attributes: config must be an AttributeConfig or None, got {config!r}")
    C = check_raster(raster)
    config.pairs(C)
    if config.confidence and probs is None:
        raise ValueError("patch_attributes: confidence needs probabilities")
    shape = tuple(raster.shape[1:])
    maps, configs, dev = checked_maps("patch_attributes", (map,), K, (patches,), device, shape)
    (labels,), (table,), _ = labelled_maps("patch_attributes", maps, K, configs, dev, shape)
    if dev is None:
        return attributes_of(labels, table, _on_host(raster), maps[0], _on_host(probs), config)
    return attributes_of(labels, table, _on_device(raster, dev), maps[0], _on_device(probs, dev), config, device=True)


def _on_host(t):
    """an array or a tensor (or None) as a host array"""
    return None if t is None else t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _on_device(t, dev):
    """an array or a tensor (or None) as a tensor on ``dev``; an array is copied first, torch wraps writable ones only"""
    import torch
    return None if t is None else (t if isinstance(t, torch.Tensor) else torch.from_numpy(np.array(t))).to(dev)
