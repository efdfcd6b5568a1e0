"""Cover grids: the share of every class (and zone) per cell of a coarser grid — 10 m cells on the lattice of a satellite
product, 100 m cells of a regional mortality map, "dead % of the forest area per cell" as ``scripts/aggregate_results.py``
of the reference computes it per tile.  A target grid is never aligned with the ortho's pixels, so the counts are
area-weighted, and they add up exactly when neighbouring rasters are merged.

The contract, shared by the host (``cover_grid_host``, numpy) and the device (``ops.cover_grid``, csrc/cover.hip):

* pixel ``(row i, col j)`` is the square ``(j, j + 1) x (i, i + 1)``, as in ``data/polygons.py``;
* a grid is two edge tables in units of 1/256 pixel (``SUBPIXEL``), ``yq[gy + 1]`` and ``xq[gx + 1]`` (int64 on the host, int32
  on the device), strictly increasing, every cell at least one pixel wide (``q[k + 1] - q[k] >= 256``: a pixel meets at most
  two cells per axis), ``|q| <= 2**23``; raster sides are at most 16384; cell ``(g, x)`` is ``[xq[x], xq[x + 1]) x
  [yq[g], yq[g + 1])`` and may overhang the raster;
* axis weights ``wy[g, i] = max(0, min(yq[g + 1], 256 (i + 1)) - max(yq[g], 256 i))`` and ``wx`` likewise (``axis_weights``);
* ``sums[g, x, z, c] = sum over (i, j) of wy[g, i] * wx[x, j] * [zones[i, j] == z and map[i, j] == c]``: int64 in units of
  1/65536 pixel; 2 <= K <= 8, 1 <= Z <= 8, without zones every pixel is zone 0; a pixel with class >= K or zone >= Z enters
  no sum and ORs 1 / 2 into an ``err`` flag, as in ``ops.zonal_counts``;
* ``area[g, x] = sum_i wy[g, i] * sum_j wx[x, j]``, the in-raster area of the cell, has a closed form (``cell_area``);
* ``gy * gx * Z * K > 2**26`` is refused.

Everything is integer after the one snap of the edges, so sums do not depend on the order: the device equals the host
under ``array_equal``, for every batch size and path.  With a previous year's map as ``zones`` the sums of a cell are its
area-weighted year-to-year transition matrix.  numpy and the standard library only."""
from __future__ import annotations

import csv
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from ..data.polygons import SUBPIXEL
from .stats import MAX_CLASSES, MAX_ZONES

MAX_SIDE = 16384
MAX_Q = 2 ** 23
MAX_SUMS = 2 ** 26
UNIT = SUBPIXEL * SUBPIXEL          # sums and areas count 1/65536 pixel


# ---------------------------------------------------------------------- edge tables
def check_edges(q, name: str = "edges") -> np.ndarray:
    """an edge table -> int64 [n + 1]; ``ValueError`` unless it is one-dimensional, integer, of two entries or more, strictly
    increasing, with every cell at least one pixel (256) wide and ``|q| <= 2**23``"""
    a = np.asarray(q)
    if a.ndim != 1 or a.size < 2 or a.dtype.kind not in "iu":
        raise ValueError(f"cover_grid: {name} must be a one-dimensional integer table of 2 entries or more, got "
                         f"{a.dtype} {a.shape}")
    a = a.astype(np.int64)
    step = np.diff(a)
    if (step <= 0).any():
        raise ValueError(f"cover_grid: {name} must be strictly increasing")
    if (step < SUBPIXEL).any():
        raise ValueError(f"cover_grid: every cell of {name} must be at least one pixel ({SUBPIXEL}) wide, got {int(step.min())}")
    if int(np.abs(a).max()) > MAX_Q:
        raise ValueError(f"cover_grid: {name} must lie within +-{MAX_Q} (1/{SUBPIXEL} pixel), got {int(np.abs(a).max())}")
    return a


def axis_weights(q, n: int) -> np.ndarray:
    """int64 [cells, n]: ``w[g, i] = max(0, min(q[g + 1], 256 (i + 1)) - max(q[g], 256 i))``, the length of pixel ``i`` of an
    axis of ``n`` pixels inside cell ``g``, in 1/256 pixel"""
    q = np.asarray(q, dtype=np.int64)
    lo = SUBPIXEL * np.arange(int(n), dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum(q[1:, None], lo + SUBPIXEL) - np.maximum(q[:-1, None], lo))


def cell_area(yq, xq, shape) -> np.ndarray:
    """int64 [gy, gx]: the in-raster area of every cell in 1/65536 pixel, ``sum_i wy[g, i] * sum_j wx[x, j]``; an axis' sum
    is the length of the cell inside ``[0, 256 n]``"""
    h, w = int(shape[0]), int(shape[1])
    yq, xq = np.asarray(yq, dtype=np.int64), np.asarray(xq, dtype=np.int64)
    ly = np.maximum(0, np.minimum(yq[1:], SUBPIXEL * h) - np.maximum(yq[:-1], 0))
    lx = np.maximum(0, np.minimum(xq[1:], SUBPIXEL * w) - np.maximum(xq[:-1], 0))
    return ly[:, None] * lx[None, :]


def check_cover(classes, zones, K, Z, yq, xq, who: str = "cover_grid"):
    """the arguments of ``cover_grid_host`` / ``ops.cover_grid`` that the host can check: shapes and dtypes of the maps (numpy
    arrays or tensors; only ``shape`` and ``dtype`` are read), K, Z, the two tables, the size bound -> ``(K, Z, yq, xq)`` with
    the tables as int64.  ``ValueError`` otherwise"""
    K, Z = int(K), int(Z)
    if not 2 <= K <= MAX_CLASSES:
        raise ValueError(f"{who}: K must be in 2..{MAX_CLASSES}, got {K}")
    if not 1 <= Z <= MAX_ZONES:
        raise ValueError(f"{who}: Z must be in 1..{MAX_ZONES}, got {Z}")
    shape = tuple(classes.shape)
    if "uint8" not in str(classes.dtype):
        raise ValueError(f"{who}: the map must be uint8, got {classes.dtype}")
    if len(shape) != 2 or min(shape) < 1 or max(shape) > MAX_SIDE:
        raise ValueError(f"{who}: the map must be [h, w] with sides in 1..{MAX_SIDE}, got {shape}")
    if zones is None:
        if Z != 1:
            raise ValueError(f"{who}: Z={Z} needs a zones map (without one every pixel is zone 0)")
    else:
        if "uint8" not in str(zones.dtype):
            raise ValueError(f"{who}: zones must be uint8, got {zones.dtype}")
        if tuple(zones.shape) != shape:
            raise ValueError(f"{who}: the map {shape} and zones {tuple(zones.shape)} must have the same shape")
    yq, xq = check_edges(yq, "yq"), check_edges(xq, "xq")
    if (len(yq) - 1) * (len(xq) - 1) * Z * K > MAX_SUMS:
        raise ValueError(f"{who}: {len(yq) - 1} x {len(xq) - 1} cells of {Z} x {K} bins are more than {MAX_SUMS} sums")
    return K, Z, yq, xq


# ---------------------------------------------------------------------- the definition
def _between_edges(a: np.ndarray, q: np.ndarray) -> np.ndarray:
    """``a`` int64 [m, n] -> int64 [m, cells]: ``sum_j w[x, j] * a[:, j]`` with ``w = axis_weights(q, n)``, without the
    matrix: the weighted sum over a cell is the integral of the row's step function between the cell's two edges, and the
    integral up to an edge ``e`` inside ``[0, 256 n]`` is ``256 * (a[:, :k].sum(1)) + r * a[:, k]`` with ``k, r = divmod(e,
    256)``"""
    m, n = a.shape
    upto = np.zeros((m, n + 1), dtype=np.int64)
    np.cumsum(a, axis=1, out=upto[:, 1:])
    e = np.clip(q, 0, SUBPIXEL * n)
    k, r = e // SUBPIXEL, e % SUBPIXEL
    at = np.concatenate([a, np.zeros((m, 1), dtype=np.int64)], axis=1)[:, k]     # r == 0 where k == n
    return np.diff(SUBPIXEL * upto[:, k] + r[None, :] * at, axis=1)


def cover_grid_host(classes, zones, K: int, Z: int, yq, xq) -> Tuple[np.ndarray, int]:
    """the definition in numpy: ``(sums int64 [gy, gx, Z, K], err)`` of a uint8 [h, w] map, ``zones`` uint8 [h, w] or None
    (Z must then be 1).  Per bin ``(z, c)`` the indicator plane is weighted along x and then along y — ``wy @ plane @ wx.T``
    with ``axis_weights``, evaluated by ``_between_edges`` so that cells of one pixel cost no more than large ones.  ``err``:
    1 when a class is >= K, 2 when a zone is >= Z (3: both); such pixels enter no sum.  ``ValueError``: see ``check_cover``"""
    classes = np.asarray(classes)
    zones = None if zones is None else np.asarray(zones)
    K, Z, yq, xq = check_cover(classes, zones, K, Z, yq, xq, "cover_grid_host")
    err = (1 if int(classes.max()) >= K else 0) | (2 if zones is not None and int(zones.max()) >= Z else 0)
    sums = np.zeros((len(yq) - 1, len(xq) - 1, Z, K), dtype=np.int64)
    for z in range(Z):
        in_zone = None if zones is None else zones == z
        for c in range(K):
            plane = classes == c if in_zone is None else (classes == c) & in_zone
            if plane.any():
                sums[:, :, z, c] = _between_edges(_between_edges(plane.astype(np.int64), xq).T.copy(), yq).T
    return sums, err


# ---------------------------------------------------------------------- the grid a caller asks for
def _pair(value, name: str, kind=float):
    if isinstance(value, (tuple, list, np.ndarray)):
        if len(value) != 2:
            raise ValueError(f"GridConfig: {name} must be a number or a pair, got {value!r}")
        pair = tuple(value)
    else:
        pair = (value, value)
    for v in pair:
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"GridConfig: {name} must hold numbers, got {value!r}")
        if kind is int and int(v) != v:
            raise ValueError(f"GridConfig: {name} must hold integers, got {value!r}")
    return tuple(kind(v) for v in pair)


def _geotransform(transform, who: str):
    t = [float(v) for v in transform]
    if len(t) != 6:
        raise ValueError(f"{who}: a GDAL geotransform has six terms (x0, dx, rx, y0, ry, dy)")
    x0, dx, rx, y0, ry, dy = t
    if rx != 0.0 or ry != 0.0:
        raise ValueError(f"{who}: rotated geotransforms are not supported (north-up only)")
    if dx == 0.0 or dy == 0.0:
        raise ValueError(f"{who}: zero pixel size")
    return x0, dx, y0, dy


@dataclass(frozen=True)
class GridConfig:
    """a regular lattice in the pixel frame of one raster: ``cell = (ch, cw)`` (or one number) and ``origin = (oy, ox)`` in
    pixels, as floats; edge ``k`` of an axis lies at ``floor((o + k * c) * 256 + 0.5)`` 1/256 pixel, computed in float64 — every
    edge is snapped individually, on the host, once, and everything behind the snap is integer.  ``index0 = (iy, ix)``: the
    global index of the cell between the edges 0 and 1.  Cells must be at least one pixel"""
    cell: object
    origin: object = (0.0, 0.0)
    index0: object = (0, 0)

    def __post_init__(self):
        object.__setattr__(self, "cell", _pair(self.cell, "cell"))
        object.__setattr__(self, "origin", _pair(self.origin, "origin"))
        object.__setattr__(self, "index0", _pair(self.index0, "index0", int))
        if not all(math.isfinite(v) for v in self.cell + self.origin):
            raise ValueError(f"GridConfig: cell and origin must be finite, got {self.cell}, {self.origin}")
        if min(self.cell) < 1.0:
            raise ValueError(f"GridConfig: a cell must be at least one pixel, got {self.cell}")
        if max(self.cell) * SUBPIXEL > MAX_Q:
            raise ValueError(f"GridConfig: a cell must be at most {MAX_Q // SUBPIXEL} pixels, got {self.cell}")

    def _axis(self, a: int, n: int):
        c, o = self.cell[a], self.origin[a]
        first = math.floor((0.0 - o) / c) - 1
        k = np.arange(first, math.ceil((n - o) / c) + 2, dtype=np.int64)
        q = np.floor((o + k.astype(np.float64) * c) * float(SUBPIXEL) + 0.5).astype(np.int64)
        inside = (q[1:] > 0) & (q[:-1] < SUBPIXEL * n)             # the cells with in-raster area: one stretch
        lo, hi = int(np.argmax(inside)), len(inside) - int(np.argmax(inside[::-1]))
        return self.index0[a] + int(k[lo]), q[lo:hi + 1]

    def edges(self, shape):
        """``(iy0, yq, ix0, xq)`` for a raster of ``shape`` (h, w): the edge tables (int64) of exactly the cells with non-zero
        in-raster area, and the global indices of the first row and column of cells.  ``ValueError`` for a table the
        contract refuses (``check_edges``: a snapped cell below one pixel, an edge beyond ``2**23``)"""
        h, w = int(shape[0]), int(shape[1])
        if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
            raise ValueError(f"GridConfig: raster sides must be in 1..{MAX_SIDE}, got {(h, w)}")
        iy0, yq = self._axis(0, h)
        ix0, xq = self._axis(1, w)
        return iy0, check_edges(yq, "yq"), ix0, check_edges(xq, "xq")

    def centre(self, iy, ix):
        """``(row, col)`` in pixels (floats, arrays allowed) of the centre of the cell with the global index ``(iy, ix)``, in
        this grid's pixel frame"""
        y = self.origin[0] + (np.asarray(iy, dtype=np.float64) - self.index0[0] + 0.5) * self.cell[0]
        x = self.origin[1] + (np.asarray(ix, dtype=np.float64) - self.index0[1] + 0.5) * self.cell[1]
        return y, x

    @classmethod
    def from_world(cls, transform, cell_m, origin_xy=(0.0, 0.0)) -> "GridConfig":
        """the world lattice ``origin_xy + k * cell_m`` (``cell_m``: one number or ``(height, width)`` in world units) in the
        pixel frame of a raster with the north-up GDAL geotransform ``(x0, dx, rx, y0, ry, dy)``; rotation raises, as in
        ``PolygonSet.to_pixels``.  Global indices ascend with the pixel rows and columns whatever the signs of ``dy`` and
        ``dx``: with ``dy < 0`` (north-up) ``iy`` runs SOUTHWARDS, cell row ``iy`` covers the world ``Y`` in ``[oy - (iy + 1) *
        ch, oy - iy * ch]``; with ``dy > 0`` it covers ``[oy + iy * ch, oy + (iy + 1) * ch]``; ``ix`` likewise (eastwards for
        ``dx > 0``).  Two rasters on one pixel lattice get the same global index for the same world cell"""
        x0, dx, y0, dy = _geotransform(transform, "GridConfig.from_world")
        ch, cw = _pair(cell_m, "cell_m")
        ox, oy = (float(v) for v in origin_xy)
        return cls(cell=(ch / abs(dy), cw / abs(dx)), origin=((oy - y0) / dy, (ox - x0) / dx))


def check_grid(option, name: str = "grid") -> Optional[GridConfig]:
    """the ``grid`` argument of ``infer_tile`` -> ``GridConfig`` or None (None: not asked for); anything else is a
    ``ValueError``"""
    if option is None:
        return None
    if isinstance(option, GridConfig):
        return option
    raise ValueError(f"{name} must be a GridConfig or None, got {option!r}")


# ---------------------------------------------------------------------- patches per cell
def bin_patches(table, yq, xq, K: int):
    """``(patch_count, patch_area)`` int64 [gy, gx, K]: the patches of a ``PatchTable`` (crowns when it is a crown table) and
    their pixels per cell and class, binned by centroid in exact integers.  A pixel's centre lies half a pixel behind its
    number, so the centre coordinate is ``(2 * sum_x + area) / (2 * area)`` pixels; it lies in cell ``k`` when ``2 * area *
    xq[k] <= 256 * (2 * sum_x + area) < 2 * area * xq[k + 1]`` (half-open) — here by the floor of the left side over ``2 *
    area``, which compares the same with integers.  A centroid outside every cell is not counted"""
    yq, xq = np.asarray(yq, dtype=np.int64), np.asarray(xq, dtype=np.int64)
    count = np.zeros((len(yq) - 1, len(xq) - 1, int(K)), dtype=np.int64)
    area = np.zeros_like(count)
    if table.n:
        a = table.area.astype(np.int64)
        g = np.searchsorted(yq, (SUBPIXEL * (2 * table.sum_y + a)) // (2 * a), side="right") - 1
        x = np.searchsorted(xq, (SUBPIXEL * (2 * table.sum_x + a)) // (2 * a), side="right") - 1
        c = table.cls.astype(np.int64)
        keep = (g >= 0) & (g < count.shape[0]) & (x >= 0) & (x < count.shape[1]) & (c < int(K))
        np.add.at(count, (g[keep], x[keep], c[keep]), 1)
        np.add.at(area, (g[keep], x[keep], c[keep]), a[keep])
    return count, area


# ---------------------------------------------------------------------- the result
def _frozen(a, dtype, shape=None, name="array"):
    a = np.array(a, dtype=dtype)
    if shape is not None and a.shape != shape:
        raise ValueError(f"CoverGrid: {name} must have shape {shape}, got {a.shape}")
    a.setflags(write=False)
    return a


class CoverGrid:
    """the cover grid of one raster, or of several merged: numpy only and read-only.  ``sums`` int64 [gy, gx, Z, K] and ``area``
    int64 [gy, gx] (the in-raster area of every cell) in 1/65536 pixel; ``full`` int64 [gy, gx]: the area of the whole cell;
    ``iy0`` / ``ix0``: the global indices of cell (0, 0); ``K`` / ``Z``; ``patch_count`` / ``patch_area`` int64 [gy, gx, K] when
    patches were asked for (``bin_patches``), else None; ``yq`` / ``xq``: the edge tables in the raster's pixel frame (None for a
    merged grid, whose rasters have different frames)"""

    def __init__(self, sums, area, iy0: int = 0, ix0: int = 0, full=None, patch_count=None, patch_area=None, yq=None, xq=None):
        sums = _frozen(sums, np.int64)
        if sums.ndim != 4 or not (1 <= sums.shape[2] <= MAX_ZONES and 2 <= sums.shape[3] <= MAX_CLASSES) or (sums < 0).any():
            raise ValueError(f"CoverGrid: sums must be non-negative [gy, gx, Z, K], got shape {sums.shape}")
        cells = sums.shape[:2]
        self._sums, self._area = sums, _frozen(area, np.int64, cells, "area")
        self.iy0, self.ix0 = int(iy0), int(ix0)
        self._yq = None if yq is None else _frozen(yq, np.int64, (cells[0] + 1,), "yq")
        self._xq = None if xq is None else _frozen(xq, np.int64, (cells[1] + 1,), "xq")
        if full is None:
            if self._yq is None or self._xq is None:
                raise ValueError("CoverGrid: the cells' full areas need `full` or both edge tables")
            full = np.diff(self._yq)[:, None] * np.diff(self._xq)[None, :]
        self._full = _frozen(full, np.int64, cells, "full")
        if (patch_count is None) != (patch_area is None):
            raise ValueError("CoverGrid: patch_count and patch_area come together")
        self._patch_count = None if patch_count is None else _frozen(patch_count, np.int64, cells + (self.K,), "patch_count")
        self._patch_area = None if patch_area is None else _frozen(patch_area, np.int64, cells + (self.K,), "patch_area")

    sums = property(lambda self: self._sums)
    area = property(lambda self: self._area)
    full = property(lambda self: self._full)
    yq = property(lambda self: self._yq)
    xq = property(lambda self: self._xq)
    patch_count = property(lambda self: self._patch_count)
    patch_area = property(lambda self: self._patch_area)
    Z = property(lambda self: self._sums.shape[2])
    K = property(lambda self: self._sums.shape[3])
    shape = property(lambda self: self._sums.shape[:2])

    @classmethod
    def of(cls, sums, edges, shape, table=None) -> "CoverGrid":
        """the grid of one raster of ``shape`` from its sums and ``edges = (iy0, yq, ix0, xq)``; ``table``: the raster's
        ``PatchTable`` for the patch figures"""
        iy0, yq, ix0, xq = edges
        count, parea = (None, None) if table is None else bin_patches(table, yq, xq, np.shape(sums)[3])
        return cls(sums, cell_area(yq, xq, shape), iy0, ix0, patch_count=count, patch_area=parea, yq=yq, xq=xq)

    def counts(self) -> np.ndarray:
        """float64 [gy, gx, Z, K]: the sums in pixels"""
        return self._sums / float(UNIT)

    def _over_area(self, num) -> np.ndarray:
        area = self._area.astype(np.float64).reshape(self._area.shape + (1,) * (num.ndim - 2))
        return np.divide(num, area, out=np.zeros(num.shape, dtype=np.float64), where=area > 0)

    def fraction(self, cls: Optional[int] = None, zone: Optional[int] = None) -> np.ndarray:
        """``sums / area``, 0 where ``area == 0``: the share of the cell's in-raster area.  ``zone``: that zone only, None: over
        all zones; ``cls``: that class -> float64 [gy, gx], None: every class -> [gy, gx, K]"""
        s = self._sums.sum(axis=2) if zone is None else self._sums[:, :, int(zone)]
        return self._over_area((s if cls is None else s[:, :, int(cls)]).astype(np.float64))

    def dead_fraction(self) -> np.ndarray:
        """float64 [gy, gx]: the share of dead pixels (classes >= 1) per cell, ``RasterStats.dead_fraction`` per cell"""
        return self._over_area(self._sums[:, :, :, 1:].sum(axis=(2, 3)).astype(np.float64))

    def forest_dead_percent(self, limit: float = 10, forest_zone: int = 1, label_weighted: bool = True) -> dict:
        """``stats.forest_dead_percent`` per cell: ``{"conifer", "broadleaf", "total"}`` as float64 [gy, gx], NaN in the cells
        with less than ``limit`` % forest (or none at all); ``label_weighted`` as there"""
        if not 0 <= forest_zone < self.Z:
            raise ValueError(f"forest_dead_percent: forest_zone {forest_zone} outside the {self.Z} zones of the grid")
        forest = self._sums[:, :, forest_zone].sum(axis=2).astype(np.float64)
        total = self._sums.sum(axis=(2, 3)).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            low = (forest == 0) | ((forest / total) * 100 < limit)
            shares = []
            for c in (1, 2):
                pixels = self._sums[:, :, forest_zone, c].astype(np.float64) if c < self.K else np.zeros_like(forest)
                shares.append(np.where(low, np.nan, ((pixels * c if label_weighted else pixels) / forest) * 100))
        return {"conifer": shares[0], "broadleaf": shares[1], "total": shares[0] + shares[1]}

    def covered(self) -> np.ndarray:
        """float64 [gy, gx]: ``area`` over the full cell area — 1 for a cell inside the raster(s), less for one that overhangs"""
        return self._area / self._full.astype(np.float64)

    def rows(self, transform=None, config: Optional[GridConfig] = None) -> List[dict]:
        """one dict per cell, row-major: ``iy``, ``ix`` (global indices), with ``transform`` (the GDAL geotransform of the pixel
        frame) the world centre ``x``, ``y``, then ``area_px`` and ``z{z}_c{c}`` in pixels (floats), and ``patches_c{c}`` /
        ``patch_px_c{c}`` when there are patch figures.  The centre is that of the edge tables, or of ``config`` (a
        ``GridConfig`` in the frame of ``transform``: the way of a merged grid)"""
        gy, gx = self.shape
        centre = None
        if transform is not None:
            x0, dx, y0, dy = _geotransform(transform, "CoverGrid.rows")
            if config is not None:
                cy, cx = config.centre(self.iy0 + np.arange(gy), self.ix0 + np.arange(gx))
            elif self._yq is not None and self._xq is not None:
                cy = (self._yq[:-1] + self._yq[1:]) / (2.0 * SUBPIXEL)
                cx = (self._xq[:-1] + self._xq[1:]) / (2.0 * SUBPIXEL)
            else:
                raise ValueError("CoverGrid.rows: a merged grid has no pixel frame of its own: pass the GridConfig of the "
                                 "raster the transform belongs to")
            centre = (y0 + cy * dy, x0 + cx * dx)
        out = []
        for g in range(gy):
            for x in range(gx):
                row = {"iy": self.iy0 + g, "ix": self.ix0 + x}
                if centre is not None:
                    row["x"], row["y"] = float(centre[1][x]), float(centre[0][g])
                row["area_px"] = int(self._area[g, x]) / UNIT
                for z in range(self.Z):
                    for c in range(self.K):
                        row[f"z{z}_c{c}"] = int(self._sums[g, x, z, c]) / UNIT
                if self._patch_count is not None:
                    for c in range(1, self.K):
                        row[f"patches_c{c}"] = int(self._patch_count[g, x, c])
                        row[f"patch_px_c{c}"] = int(self._patch_area[g, x, c])
                out.append(row)
        return out

    @classmethod
    def merge(cls, grids: Sequence["CoverGrid"]) -> "CoverGrid":
        """the grid of several rasters: ``sums``, ``area`` and the patch figures are added by global cell index into the
        bounding index box (``full`` is taken where a grid has the cell).  ``ValueError`` for differing ``K`` / ``Z`` or no
        grid.  This is EXACT — equal to the grid of the mosaic — when the rasters' snaps of every shared edge agree, i.e. when
        the edge lies at the same place in both pixel frames; rasters offset by whole pixels with cell sizes and origins that
        float64 represents exactly (so that ``origin + k * cell`` rounds nowhere) do.  The patch figures add patches per
        raster: a patch cut by the seam counts once on either side"""
        grids = list(grids)
        if not grids:
            raise ValueError("CoverGrid.merge: no grid")
        first = grids[0]
        for g in grids:
            if not isinstance(g, CoverGrid):
                raise ValueError(f"CoverGrid.merge: not a CoverGrid: {type(g).__name__}")
            if (g.K, g.Z) != (first.K, first.Z):
                raise ValueError(f"CoverGrid.merge: K / Z differ: {(g.K, g.Z)} against {(first.K, first.Z)}")
        iy0, ix0 = min(g.iy0 for g in grids), min(g.ix0 for g in grids)
        gy = max(g.iy0 + g.shape[0] for g in grids) - iy0
        gx = max(g.ix0 + g.shape[1] for g in grids) - ix0
        if gy * gx * first.Z * first.K > MAX_SUMS:
            raise ValueError(f"CoverGrid.merge: {gy} x {gx} cells are more than {MAX_SUMS} sums")
        sums = np.zeros((gy, gx, first.Z, first.K), dtype=np.int64)
        area, full = np.zeros((gy, gx), dtype=np.int64), np.zeros((gy, gx), dtype=np.int64)
        with_patches = all(g.patch_count is not None for g in grids)
        count = np.zeros((gy, gx, first.K), dtype=np.int64) if with_patches else None
        parea = np.zeros((gy, gx, first.K), dtype=np.int64) if with_patches else None
        for g in grids:
            box = (slice(g.iy0 - iy0, g.iy0 - iy0 + g.shape[0]), slice(g.ix0 - ix0, g.ix0 - ix0 + g.shape[1]))
            sums[box] += g.sums
            area[box] += g.area
            full[box] = np.maximum(full[box], g.full)
            if with_patches:
                count[box] += g.patch_count
                parea[box] += g.patch_area
        return cls(sums, area, iy0, ix0, full=full, patch_count=count, patch_area=parea)

    def __eq__(self, other) -> bool:
        if not isinstance(other, CoverGrid):
            return NotImplemented
        if (self.iy0, self.ix0) != (other.iy0, other.ix0) or (self._patch_count is None) != (other._patch_count is None):
            return False
        names = ["_sums", "_area", "_full"] + ([] if self._patch_count is None else ["_patch_count", "_patch_area"])
        return all(np.array_equal(getattr(self, n), getattr(other, n)) for n in names)

    __hash__ = None

    def __repr__(self) -> str:
        tail = "" if self._patch_count is None else f", patches={int(self._patch_count.sum())}"
        return (f"CoverGrid({self.shape[0]} x {self.shape[1]} cells from ({self.iy0}, {self.ix0}), Z={self.Z}, K={self.K}, "
                f"area_px={int(self._area.sum()) / UNIT!r}{tail})")


def write_cover_csv(path, grid: CoverGrid, transform=None, config: Optional[GridConfig] = None) -> None:
    """``CoverGrid.rows`` through the ``csv`` module, one line per cell"""
    table = grid.rows(transform, config)
    with open(path, "w", newline="") as f:
        writer = csv.DictWriter(f, fieldnames=list(table[0]))
        writer.writeheader()
        writer.writerows(table)


def cover_grid(classes, K: int, grid: GridConfig, zones=None, device=None, n_zones: Optional[int] = None) -> CoverGrid:
    """the ``CoverGrid`` of any uint8 [h, w] class map under a ``GridConfig``: a numpy array (computed by ``cover_grid_host``,
    or uploaded when ``device`` names a HIP device) or a tensor (on a HIP device by ``ops.cover_grid``, on the CPU by the
    host contract).  ``zones``: uint8 [h, w] of the same kind, or None; ``n_zones`` defaults to ``zones.max() + 1``.  A value out
    of range is a ``ValueError``"""
    grid = check_grid(grid)
    if grid is None:
        raise ValueError("cover_grid: grid must be a GridConfig")
    import torch
    tensors = isinstance(classes, torch.Tensor)
    if zones is not None and isinstance(zones, torch.Tensor) != tensors:
        raise ValueError("cover_grid: the map and zones must both be arrays or both be tensors")
    if not tensors:
        classes = np.asarray(classes)
        zones = None if zones is None else np.asarray(zones)
    if zones is None:
        Z = 1 if n_zones is None else int(n_zones)
    else:
        Z = int(zones.max()) + 1 if n_zones is None else int(n_zones)
    if len(classes.shape) != 2:
        raise ValueError(f"cover_grid: the map must be [h, w], got {tuple(classes.shape)}")
    edges = grid.edges(classes.shape)
    K, Z, yq, xq = check_cover(classes, zones, K, Z, edges[1], edges[3])
    on_device = (tensors and classes.is_cuda) or (device is not None and str(device).startswith("cuda"))
    if on_device:
        from .. import ops
        if not tensors:
            classes = torch.from_numpy(np.ascontiguousarray(classes)).to(device)
            zones = None if zones is None else torch.from_numpy(np.ascontiguousarray(zones)).to(device)
        sums, err = ops.cover_grid(classes, zones, K, Z, yq, xq)
        sums, err = sums.cpu().numpy(), int(err.cpu())
    else:
        sums, err = cover_grid_host(classes.numpy() if tensors else classes, None if zones is None else
                                    (zones.numpy() if tensors else zones), K, Z, yq, xq)
    if err:
        raise ValueError(f"cover_grid: a value out of range (flag {err}: 1 class >= {K}, 2 zone >= {Z})")
    return CoverGrid.of(sums, edges, tuple(classes.shape))
