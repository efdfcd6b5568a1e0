"""Masks and zones from polygons: exact all-touched rasterisation.

The reference burns the annotators' polygons into per-tile masks off line (``scripts/createmasks.py``: a shapefile with a
``type`` column, ``rio.clip(..., all_touched=True)`` once per class, ``argmax`` over ``[0, conifer, broadleaf]``), which
needs GDAL / geopandas.  Here the rule is stated once in integers and computed on the host in numpy (``rasterize_host``:
the CPU path and the yardstick of the GPU tests) and on the device (csrc/polygons.hip through ``ops.rasterize_polygons``),
bit for bit the same.

Contract:
  grid    pixel coordinates, x along columns, y along rows; pixel (row i, col j) is the square (j, j+1) x (i, i+1) and its
          centre is (j + 0.5, i + 0.5).  Every vertex is snapped once, on the host, to 1/256 pixel: ``q = floor(v * 256 +
          0.5)`` in float64, stored as int32, ``|q| <= 2^23``; raster sides <= 16384.  Everything after that is integer
          arithmetic: coordinate differences fit int32, a cross product is one 32 x 32 -> 64 multiply-add.
  burn    a polygon (exterior ring + hole rings, even-odd parity over all its rings) burns a pixel iff
          centre  the pixel centre c is inside: the crossing number of the ray to +x with the half-open rule ``(ay <= cy)
                  != (by <= cy)``; a crossing lies on the ray iff ``cross(b - a, c - a)`` of the edge taken upwards is > 0;
          touch   (``all_touched=True``) some ring segment meets the pixel's OPEN square: its bounding box strictly
                  overlaps the square in x and in y, and the cross products of the four corners against the segment
                  satisfy ``min < 0 < max``.  Zero-length segments are skipped.
  values  every polygon carries a uint8 value in 1..255; a pixel gets the MINIMUM value among the polygons that burn it,
          0 if none does.  With class ids this is the reference's argmax (class 1 wins over class 2), with ones it is
          ``--simple``, with zone ids a deterministic overlap rule.

This restates GDAL's published ``ALL_TOUCHED`` behaviour (a scanline fill at pixel centres plus every pixel a ring line
passes through); the deliberate difference is on measure-zero input: a segment lying exactly on a pixel grid line burns
neither neighbour by the touch rule.  Parity with rasterio is unpinned: rasterio, shapely and geopandas are not available
to the tests.
"""
from __future__ import annotations

import csv
import json
import os
from typing import Iterable, Optional, Sequence, Tuple

import numpy as np

SUBPIXEL = 256                # fixed-point units per pixel
COORD_LIMIT = 1 << 23         # |q| bound of a snapped coordinate
MAX_SIDE = 16384              # raster sides
POLY_COLS = 8                 # columns of the device polygon table: minx, miny, maxx, maxy, e0, e1, value, 0


def snap(v) -> np.ndarray:
    """pixel coordinates -> the fixed-point grid: ``floor(v * 256 + 0.5)`` in float64 as int64 (the bound is checked by
    ``PolygonSet``)"""
    v = np.asarray(v, dtype=np.float64)
    if not np.all(np.isfinite(v)):
        raise ValueError("polygon coordinates must be finite")
    q = np.floor(v * SUBPIXEL + 0.5)
    if q.size and float(np.abs(q).max()) > COORD_LIMIT:
        raise ValueError(f"polygon coordinate outside +-{COORD_LIMIT // SUBPIXEL} pixels (|q| <= 2^23 at 1/256 pixel)")
    return q.astype(np.int64)


def _ring(ring) -> np.ndarray:
    r = np.asarray(ring, dtype=np.float64)
    if r.ndim != 2 or r.shape[1] < 2:
        raise ValueError(f"a ring is a sequence of (x, y) pairs, not shape {r.shape}")
    r = r[:, :2]
    if len(r) >= 2 and np.array_equal(r[0], r[-1]):        # a closed ring (GeoJSON repeats the first vertex)
        r = r[:-1]
    if len(r) < 3:
        raise ValueError(f"a ring needs at least 3 vertices, got {len(r)}")
    return r


class PolygonSet:
    """Polygons on a fixed-point pixel grid (or, from ``from_geojson``, still in world coordinates: ``to_pixels`` snaps
    them).  Immutable; validated at construction (``ValueError``).

    ``xy`` int32 [V, 2] snapped vertices (x, y) of all rings; ``ring_offsets`` int64 [R + 1]; ``ring_polygon`` int32 [R]
    (non-decreasing: a polygon's exterior ring, then its holes); ``values`` uint8 [P] in 1..255; ``bounds`` int32 [P, 4]
    (minx, miny, maxx, maxy over the polygon's vertices)."""

    def __init__(self, xy, ring_offsets, ring_polygon, values):
        xy = np.asarray(xy)
        if xy.ndim != 2 or xy.shape[1] != 2 or not np.issubdtype(xy.dtype, np.integer):
            raise ValueError(f"PolygonSet: xy must be integer [V, 2] (snapped vertices), not {xy.dtype} {xy.shape}")
        if xy.size and int(np.abs(xy.astype(np.int64)).max()) > COORD_LIMIT:
            raise ValueError(f"PolygonSet: snapped coordinate outside |q| <= 2^23")
        ro = np.asarray(ring_offsets, dtype=np.int64).reshape(-1)
        rp = np.asarray(ring_polygon, dtype=np.int64).reshape(-1)
        vals = np.asarray(values)
        if vals.ndim != 1:
            raise ValueError("PolygonSet: values must be one per polygon")
        if vals.size and (not np.all(vals == np.floor(vals)) or vals.min() < 1 or vals.max() > 255):
            raise ValueError("PolygonSet: polygon values must be integers in 1..255")
        P, R = len(vals), len(rp)
        if len(ro) != R + 1 or ro[0] != 0 or ro[-1] != len(xy):
            raise ValueError("PolygonSet: ring_offsets must run from 0 to the vertex count, one entry per ring plus one")
        if R and int(np.diff(ro).min()) < 3:
            raise ValueError("PolygonSet: a ring needs at least 3 vertices")
        if R and (rp[0] != 0 or rp[-1] != P - 1 or np.any(np.diff(rp) < 0) or np.any(np.diff(rp) > 1)):
            raise ValueError("PolygonSet: ring_polygon must name every polygon, in order")
        if not R and P:
            raise ValueError("PolygonSet: a polygon without rings")
        self._xy = xy.astype(np.int32)
        self._ring_offsets, self._ring_polygon = ro, rp.astype(np.int32)
        self._values = vals.astype(np.uint8)
        first = np.searchsorted(rp, np.arange(P + 1))                 # first ring of every polygon
        self._poly_vertices = ro[first]                               # int64 [P + 1]: vertex range of every polygon
        b = np.zeros((P, 4), np.int32)
        if P:
            at = self._poly_vertices[:-1]
            b[:, 0] = np.minimum.reduceat(self._xy[:, 0], at)
            b[:, 1] = np.minimum.reduceat(self._xy[:, 1], at)
            b[:, 2] = np.maximum.reduceat(self._xy[:, 0], at)
            b[:, 3] = np.maximum.reduceat(self._xy[:, 1], at)
        self._bounds = b
        for a in (self._xy, self._ring_offsets, self._ring_polygon, self._values, self._bounds, self._poly_vertices):
            a.setflags(write=False)
        self._tables = None
        self._world = None            # from_geojson: (float64 [V, 2] world coordinates) until to_pixels

    xy = property(lambda self: self._xy)
    ring_offsets = property(lambda self: self._ring_offsets)
    ring_polygon = property(lambda self: self._ring_polygon)
    values = property(lambda self: self._values)
    bounds = property(lambda self: self._bounds)

    def __len__(self) -> int:
        return len(self._values)

    def __repr__(self) -> str:
        return f"PolygonSet({len(self)} polygons, {len(self._ring_polygon)} rings, {len(self._xy)} vertices)"

    # ------------------------------------------------------------------------------------------ constructors
    @classmethod
    def _from_rings(cls, polygons, world: bool = False) -> "PolygonSet":
        rings, rp, values = [], [], []
        for p, poly in enumerate(polygons):
            if len(poly) not in (2, 3):
                raise ValueError("a polygon is (value, exterior) or (value, exterior, [holes...])")
            value, exterior = poly[0], poly[1]
            holes = poly[2] if len(poly) == 3 and poly[2] is not None else []
            for r in [exterior, *holes]:
                rings.append(_ring(r))
                rp.append(p)
            values.append(value)
        coords = np.concatenate(rings) if rings else np.zeros((0, 2), np.float64)
        ro = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int64)
        if world:
            out = cls(np.zeros((len(coords), 2), np.int32), ro, rp, values)
            out._world = coords
            return out
        return cls(snap(coords), ro, rp, values)

    @classmethod
    def from_polygons(cls, polygons: Iterable) -> "PolygonSet":
        """``[(value, exterior, [holes...]), ...]`` in pixel coordinates; rings are sequences of (x, y), closed or not"""
        return cls._from_rings(polygons)

    @classmethod
    def from_geojson(cls, obj_or_path, value_property: str = "type", simple: bool = False,
                     keep_values: Optional[Sequence[int]] = (1, 2)) -> "PolygonSet":
        """A GeoJSON ``FeatureCollection`` of ``Polygon`` / ``MultiPolygon`` features (a dict, a JSON string or a path) in
        the file's own coordinates: follow with ``to_pixels(transform)``.  Multi-polygons are exploded; any other
        geometry type raises ``ValueError``.  The value is ``int(float(properties[value_property]))`` (the capitalised
        name answers too: the reference renames ``type`` to ``Type``); features whose value is not in ``keep_values``
        are dropped (None keeps all); ``simple=True`` gives every kept polygon the value 1."""
        obj = obj_or_path
        if isinstance(obj, (str, bytes, os.PathLike)):
            text = obj.decode() if isinstance(obj, bytes) else obj
            if isinstance(text, str) and text.lstrip().startswith("{"):
                obj = json.loads(text)
            else:
                with open(os.fspath(text)) as f:
                    obj = json.load(f)
        if not isinstance(obj, dict) or obj.get("type") != "FeatureCollection":
            raise ValueError("from_geojson: expected a GeoJSON FeatureCollection")
        names = (value_property, value_property.capitalize(), value_property.lower())
        polygons = []
        for k, feat in enumerate(obj.get("features", [])):
            geom = feat.get("geometry") or {}
            kind = geom.get("type")
            if kind == "Polygon":
                parts = [geom["coordinates"]]
            elif kind == "MultiPolygon":
                parts = list(geom["coordinates"])
            else:
                raise ValueError(f"from_geojson: feature {k} is a {kind}; only Polygon and MultiPolygon are rasterised")
            props = feat.get("properties") or {}
            name = next((n for n in names if n in props), None)
            if name is None:
                raise ValueError(f"from_geojson: feature {k} has no {value_property!r} property")
            try:
                value = int(float(props[name]))
            except (TypeError, ValueError):
                raise ValueError(f"from_geojson: feature {k}: {name}={props[name]!r} is not a number") from None
            if keep_values is not None and value not in keep_values:
                continue
            for rings in parts:
                if not rings:
                    raise ValueError(f"from_geojson: feature {k} has a polygon without rings")
                polygons.append((1 if simple else value, rings[0], list(rings[1:])))
        return cls._from_rings(polygons, world=True)

    # ------------------------------------------------------------------------------------------ geometry
    def _need_pixels(self, what: str) -> None:
        if self._world is not None:
            raise ValueError(f"{what}: these polygons are in world coordinates; call to_pixels(transform) first")

    def to_pixels(self, transform) -> "PolygonSet":
        """world coordinates -> the pixel grid of a raster with GDAL geotransform ``(x0, dx, rx, y0, ry, dy)``: column =
        (X - x0) / dx, row = (Y - y0) / dy (north-up: dy < 0), snapped.  Rotation terms other than zero raise
        ``ValueError``.  A set that is already in pixel coordinates is mapped likewise (its coordinates read as world)."""
        t = [float(v) for v in transform]
        if len(t) != 6:
            raise ValueError("to_pixels: a GDAL geotransform has six terms (x0, dx, rx, y0, ry, dy)")
        x0, dx, rx, y0, ry, dy = t
        if rx != 0.0 or ry != 0.0:
            raise ValueError("to_pixels: rotated geotransforms are not supported (north-up only)")
        if dx == 0.0 or dy == 0.0:
            raise ValueError("to_pixels: zero pixel size")
        world = self._world if self._world is not None else self._xy.astype(np.float64) / SUBPIXEL
        px = np.stack([(world[:, 0] - x0) / dx, (world[:, 1] - y0) / dy], axis=1)
        return PolygonSet(snap(px), self._ring_offsets, self._ring_polygon, self._values)

    def select(self, keep) -> "PolygonSet":
        """the polygons ``keep`` (bool [P]) marks, in order"""
        keep = np.asarray(keep, dtype=bool)
        if keep.shape != (len(self),):
            raise ValueError(f"select: keep must be bool [{len(self)}]")
        ring_keep = keep[self._ring_polygon] if len(self._ring_polygon) else np.zeros(0, bool)
        lens = np.diff(self._ring_offsets)
        vert_keep = np.repeat(ring_keep, lens)
        new_id = np.cumsum(keep) - 1
        out = PolygonSet(self._xy[vert_keep], np.concatenate([[0], np.cumsum(lens[ring_keep])]),
                         new_id[self._ring_polygon[ring_keep]], self._values[keep])
        if self._world is not None:
            out._world = self._world[vert_keep]
        return out

    def clip_to(self, h: int, w: int) -> "PolygonSet":
        """drops the polygons whose bounding box misses the raster's open extent (0, w) x (0, h): they burn nothing"""
        self._need_pixels("clip_to")
        b = self._bounds.astype(np.int64)
        return self.select((b[:, 0] < int(w) * SUBPIXEL) & (b[:, 2] > 0) & (b[:, 1] < int(h) * SUBPIXEL) & (b[:, 3] > 0))

    def tables(self) -> Tuple[np.ndarray, np.ndarray]:
        """what the rule walks, on the host and on the device: ``edges`` int32 [E, 4] rows (ax, ay, bx, by), every ring
        closed, taken upwards (ay < by, or ay == by and ax < bx; neither rule depends on the direction), zero-length
        segments left out; ``polys`` int32 [P, 8] rows (minx, miny, maxx, maxy, e0, e1, value, 0) with the polygon's
        edges ``e0 .. e1``"""
        self._need_pixels("rasterize")
        if self._tables is None:
            V, P = len(self._xy), len(self)
            nxt = np.arange(1, V + 1, dtype=np.int64)
            nxt[self._ring_offsets[1:] - 1] = self._ring_offsets[:-1]
            a, b = self._xy.astype(np.int64), self._xy[nxt[:V]].astype(np.int64)
            flip = (a[:, 1] > b[:, 1]) | ((a[:, 1] == b[:, 1]) & (a[:, 0] > b[:, 0]))
            a, b = np.where(flip[:, None], b, a), np.where(flip[:, None], a, b)
            live = np.any(a != b, axis=1)
            edges = np.concatenate([a, b], axis=1)[live].astype(np.int32)
            before = np.concatenate([[0], np.cumsum(live)])            # live edges before vertex v
            polys = np.zeros((P, POLY_COLS), np.int32)
            polys[:, :4] = self._bounds
            polys[:, 4] = before[self._poly_vertices[:-1]]
            polys[:, 5] = before[self._poly_vertices[1:]]
            polys[:, 6] = self._values
            edges.setflags(write=False)
            polys.setflags(write=False)
            self._tables = (np.ascontiguousarray(edges), polys)
        return self._tables


# ---------------------------------------------------------------------------------------------- locations.csv
def read_locations_csv(path) -> dict:
    """the reference's ``locations.csv`` (``;``-separated, no header: ``filename;x1;x2;y1;y2``) -> ``{filename: (x1, x2,
    y1, y2)}`` as floats"""
    out = {}
    with open(os.fspath(path), newline="") as f:
        for n, row in enumerate(csv.reader(f, delimiter=";")):
            if not row or all(not c.strip() for c in row):
                continue
            if len(row) != 5:
                raise ValueError(f"{path}: line {n + 1}: expected filename;x1;x2;y1;y2, got {len(row)} fields")
            try:
                out[row[0].strip()] = tuple(float(c) for c in row[1:])
            except ValueError:
                raise ValueError(f"{path}: line {n + 1}: extent is not numeric: {row[1:]}") from None
    return out


def tile_transform(x1: float, x2: float, y1: float, y2: float, h: int, w: int) -> tuple:
    """the north-up GDAL geotransform of an h x w tile that covers x1..x2 (west to east) and y1..y2 (either order: the top
    row is the larger y)"""
    x1, x2, y1, y2 = float(x1), float(x2), float(y1), float(y2)
    if x2 <= x1 or y1 == y2 or h < 1 or w < 1:
        raise ValueError(f"tile_transform: empty extent x {x1}..{x2}, y {y1}..{y2} or raster {h}x{w}")
    top, bottom = max(y1, y2), min(y1, y2)
    return (x1, (x2 - x1) / w, 0.0, top, 0.0, (bottom - top) / h)


# ---------------------------------------------------------------------------------------------- the rule in numpy
def _check_raster(h, w) -> Tuple[int, int]:
    h, w = int(h), int(w)
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"rasterize: raster {h}x{w} must be 1..{MAX_SIDE} in height and width")
    return h, w


def _centre_rows(e, h, w, r0, nr, c0, nc) -> np.ndarray:
    """bool [nr, nc]: the pixels of the window whose centre is inside (even-odd over the edges e int64 [n, 4])"""
    ax, ay, bx, by = e[:, 0], e[:, 1], e[:, 2], e[:, 3]
    half = SUBPIXEL // 2
    # rows whose centre line cy = 256 i + 128 the (upward) edge crosses: ay <= cy < by
    i0 = np.maximum(-((half - ay) // SUBPIXEL), r0)
    i1 = np.minimum(-((half - by) // SUBPIXEL), r0 + nr)                   # exclusive
    n = np.maximum(i1 - i0, 0)
    which = np.repeat(np.arange(len(e)), n)
    if not len(which):
        return np.zeros((nr, nc), bool)
    start = np.cumsum(n) - n
    i = i0[which] + (np.arange(len(which)) - start[which])
    cy = i * SUBPIXEL + half
    # the crossing lies on the ray from cx iff D (cx - ax) < N, N = (bx - ax)(cy - ay), D = by - ay > 0
    D = (by - ay)[which]
    N = (bx - ax)[which] * (cy - ay[which])
    xlim = ax[which] - ((-N) // D) - 1                                     # the largest integer cx that satisfies it
    k = np.clip((xlim - half) // SUBPIXEL + 1 - c0, 0, nc)                 # columns c0 .. c0 + k - 1 flip
    cnt = np.zeros((nr, nc + 1), np.int64)
    np.add.at(cnt, (i - r0, k), 1)
    above = np.cumsum(cnt[:, ::-1], axis=1)[:, ::-1]                       # crossings with k > j, at column j
    return (above[:, 1:] & 1).astype(bool)


def _touch_pixels(e, r0, nr, c0, nc) -> np.ndarray:
    """bool [nr, nc]: the pixels of the window whose open square some edge of e meets"""
    out = np.zeros((nr, nc), bool)
    ax, ay, bx, by = e[:, 0], e[:, 1], e[:, 2], e[:, 3]
    # rows whose open slab (256 i, 256 i + 256) the edge's y range strictly overlaps
    i0 = np.maximum(ay // SUBPIXEL, r0)
    i1 = np.minimum(-((-by) // SUBPIXEL), r0 + nr)
    n = np.maximum(i1 - i0, 0)
    which = np.repeat(np.arange(len(e)), n)
    if not len(which):
        return out
    start = np.cumsum(n) - n
    i = i0[which] + (np.arange(len(which)) - start[which])
    eax, eay, ebx, eby = ax[which], ay[which], bx[which], by[which]
    D = eby - eay
    # a conservative column range: x of the edge at the two ends of its part inside the slab (exact test below)
    ylo, yhi = np.maximum(eay, i * SUBPIXEL), np.minimum(eby, (i + 1) * SUBPIXEL)
    Ds = np.where(D == 0, 1, D)
    xa = np.where(D == 0, eax, eax + ((ebx - eax) * (ylo - eay)) // Ds)
    xb = np.where(D == 0, ebx, eax + ((ebx - eax) * (yhi - eay)) // Ds)
    j0 = np.maximum(np.minimum(xa, xb) // SUBPIXEL, c0)
    j1 = np.minimum((np.maximum(xa, xb) + 1) // SUBPIXEL + 1, c0 + nc)     # exclusive
    m = np.maximum(j1 - j0, 0)
    pair = np.repeat(np.arange(len(which)), m)
    if not len(pair):
        return out
    pstart = np.cumsum(m) - m
    j = j0[pair] + (np.arange(len(pair)) - pstart[pair])
    i = i[pair]
    eax, eay, ebx, eby = eax[pair], eay[pair], ebx[pair], eby[pair]
    X0, Y0 = j * SUBPIXEL, i * SUBPIXEL
    X1, Y1 = X0 + SUBPIXEL, Y0 + SUBPIXEL
    box = (np.minimum(eax, ebx) < X1) & (np.maximum(eax, ebx) > X0) & (eay < Y1) & (eby > Y0)
    ux, uy = ebx - eax, eby - eay
    c00 = ux * (Y0 - eay) - uy * (X0 - eax)
    c10 = c00 - uy * SUBPIXEL
    c01 = c00 + ux * SUBPIXEL
    c11 = c01 - uy * SUBPIXEL
    lo = np.minimum(np.minimum(c00, c10), np.minimum(c01, c11))
    hi = np.maximum(np.maximum(c00, c10), np.maximum(c01, c11))
    hit = box & (lo < 0) & (hi > 0)
    out[i[hit] - r0, j[hit] - c0] = True
    return out


def rasterize_host(polys: PolygonSet, h: int, w: int, all_touched: bool = True) -> np.ndarray:
    """The contract in vectorised int64 numpy: uint8 [h, w], the minimum value among the polygons that burn a pixel, 0
    where none does.  A scanline form of the rule (per edge and centre line the exact last column the crossing lies to
    the right of; per edge and pixel row the exact corner test on the columns the edge passes), one polygon at a time
    inside its bounding box."""
    h, w = _check_raster(h, w)
    edges, table = polys.tables()
    edges = edges.astype(np.int64)
    out = np.zeros((h, w), np.uint8)
    for row in table.astype(np.int64):
        minx, miny, maxx, maxy, e0, e1, value = row[:7]
        # the pixels whose open square the bounding box strictly overlaps: nothing else can burn
        r0, r1 = max(miny // SUBPIXEL, 0), min(-((-maxy) // SUBPIXEL), h)
        c0, c1 = max(minx // SUBPIXEL, 0), min(-((-maxx) // SUBPIXEL), w)
        if r1 <= r0 or c1 <= c0 or e1 <= e0:
            continue
        e = edges[e0:e1]
        burn = _centre_rows(e, h, w, r0, r1 - r0, c0, c1 - c0)
        if all_touched:
            burn |= _touch_pixels(e, r0, r1 - r0, c0, c1 - c0)
        win = out[r0:r1, c0:c1]
        np.copyto(win, np.uint8(value), where=burn & ((win == 0) | (win > value)))
    return out


def rasterize(polys: PolygonSet, shape, device=None, all_touched: bool = True, out=None):
    """``polys`` burnt into a uint8 [h, w] map: on a HIP device (``device`` a ``cuda`` device, or ``out`` a tensor on
    one) by ``ops.rasterize_polygons`` — the tables are uploaded, the map is a device tensor, ``out`` may be a contiguous
    view into a larger buffer — otherwise by ``rasterize_host`` (a numpy array; ``out``: a uint8 [h, w] array that is
    overwritten)."""
    import torch
    h, w = _check_raster(*shape)
    if not isinstance(polys, PolygonSet):
        raise ValueError(f"rasterize: expected a PolygonSet, got {type(polys).__name__}")
    dev = out.device if isinstance(out, torch.Tensor) else (None if device is None else torch.device(device))
    if dev is not None and dev.type == "cuda":
        from .. import ops
        edges, table = polys.tables()
        # (the cached tables are read-only; torch wraps writable memory)
        return ops.rasterize_polygons(torch.from_numpy(edges.copy()).to(dev), torch.from_numpy(table.copy()).to(dev), (h, w),
                                      all_touched=all_touched, out=out)
    res = rasterize_host(polys, h, w, all_touched)
    if out is None:
        return res
    if isinstance(out, torch.Tensor):
        if out.dtype != torch.uint8 or tuple(out.shape) != (h, w):
            raise ValueError(f"rasterize: out must be uint8 [{h},{w}]")
        out.copy_(torch.from_numpy(res))
        return out
    if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or out.shape != (h, w):
        raise ValueError(f"rasterize: out must be uint8 [{h},{w}]")
    out[...] = res
    return out
