"""Dead-tree patch outlines: the vector layer of a predicted class map — one polygon per patch of ``deployment/patches.py``,
traced exactly along the pixel edges, as a ``PolygonSet`` (``data/polygons.py``) and as GeoJSON.

The contract, in one place (the device path, ``csrc/outlines.hip`` through ``ops.patch_outlines``, computes
exactly this; ``polygonize_host`` is the CPU path and the tests' yardstick).  It is stated on the label plane ``L`` of
``label_patches_host`` / ``ops.label_patches`` (after the sieve, if any); ``L`` counts as 0 outside the raster.

* **grid**: pixel (row i, col j) is the square (j, j+1) x (i, i+1) as in ``data/polygons.py``; vertices are the integer
  grid points (x, y), 0 <= x <= w, 0 <= y <= h;
* **boundary edges**: a labelled pixel ``p = i * w + j`` owns side ``s`` iff the neighbour across that side carries
  another label (background, another patch and the raster edge alike).  Sides are directed so that the patch lies on the
  right-hand side of the walk (y points down): 0 top (j,i)->(j+1,i) E, 1 right (j+1,i)->(j+1,i+1) S, 2 bottom
  (j+1,i+1)->(j,i+1) W, 3 left (j,i+1)->(j,i) N.  The edge key is ``4 * p + s``;
* **successor** of edge (p, s) with label l; B is the pixel ahead of p in the heading direction, A is B's neighbour
  across side s (ahead-left):
  connectivity 8: ``L[A] == l`` -> (A, (s+3)%4) left; else ``L[B] == l`` -> (B, s) straight; else (p, (s+1)%4) right;
  connectivity 4: ``L[B] != l`` -> (p, (s+1)%4) right; else ``L[A] != l`` -> (B, s) straight; else (A, (s+3)%4) left.
  The successor is a bijection on the edges and its cycles are the rings; at a saddle vertex an 8-connected patch passes
  through the diagonal (its ring touches itself there), a 4-connected one turns tight;
* **canonical form**: a ring's id is the smallest edge key on its cycle; its vertices are the end points of the edges
  whose successor has another side (the corners), in cycle order from the id edge on, not closed.  The rings of a patch
  are those whose id edge belongs to one of its pixels: ``4 * root + 0`` is the exterior (positive shoelace area in pixel
  coordinates), all others are holes (negative area) in ascending id.  Polygons come in ascending root: polygon ``k`` is
  row ``k`` of the ``PatchTable`` of the same label plane, its value the patch's class;
* **result**: ``PolygonSet(xy = 256 * vertices, ring_offsets, ring_polygon, values)`` straight from the integer arrays (no
  snapping); a map without a patch gives the empty set.  ``rasterize_host(polygonize_host(map), h, w, all_touched=False)``
  is ``map`` again, byte for byte.

numpy only (``label_patches_host`` imports scipy lazily).
"""
from __future__ import annotations

import json
import os
from typing import Optional

import numpy as np

from ..data.polygons import MAX_SIDE, SUBPIXEL, PolygonSet
from .patches import PatchConfig, PatchTable, _check_labels, _check_map, label_patches_host
from .stats import MAX_CLASSES

# pixel offsets (di, dj): the neighbour across side s, the pixel B ahead of side s, and A = B's neighbour across side s
_ACROSS = np.array([(-1, 0), (0, 1), (1, 0), (0, -1)], np.int64)
_AHEAD = np.array([(0, 1), (1, 0), (0, -1), (-1, 0)], np.int64)
_AHEAD_LEFT = _ACROSS + _AHEAD
# end point of side s relative to the pixel's (j, i)
_END_X = np.array([1, 1, 0, 0], np.int64)
_END_Y = np.array([0, 1, 1, 0], np.int64)
_POPCOUNT = np.array([bin(m).count("1") for m in range(16)], np.uint8)
# owned sides below side t in a 4-bit side mask: the place of (p, t) among the edges of p
_POP_LOW = np.array([[bin(m & ((1 << t) - 1)).count("1") for t in range(4)] for m in range(16)], np.int64)


def empty_outlines() -> PolygonSet:
    """the outlines of a map without a patch"""
    return PolygonSet(np.zeros((0, 2), np.int32), [0], [], np.zeros(0, np.uint8))


def _jump(succ: np.ndarray, corner: np.ndarray):
    """pointer jumping over the successor permutation: (m, d) per edge — m the smallest edge on the edge's cycle, d the
    number of corners from the edge forward to edge m, m itself excluded.  Per edge the state (m, d, ws, j) starts as
    (e, 0, corner(e), succ(e)) and stands for the window of 2^k edges from e on: its minimum, the corners before the
    minimum's first occurrence, the corners of the whole window, and the edge behind it.  A window that wraps around its
    cycle does no harm: min is idempotent and the strict ``<`` keeps the first occurrence"""
    E = len(succ)
    m = np.arange(E, dtype=np.int32)
    d = np.zeros(E, np.int32)
    ws = corner.astype(np.int32)
    j = succ.astype(np.int32)
    for _ in range(max(E - 1, 0).bit_length()):              # ceil(log2(E)) rounds
        mj = m[j]
        lower = mj < m
        d = np.where(lower, ws + d[j], d)
        m = np.where(lower, mj, m)
        ws = ws + ws[j]
        j = j[j]
    return m, d


def outlines_from_labels(labels: np.ndarray, classes_u8: np.ndarray, connectivity: int) -> PolygonSet:
    """the module's contract on a label plane and its class map (both already checked)"""
    h, w = labels.shape
    pad = np.zeros((h + 2, w + 2), np.int32)
    pad[1:-1, 1:-1] = labels
    centre = pad[1:-1, 1:-1]
    mask = np.zeros((h, w), np.uint8)
    for s, (di, dj) in enumerate(_ACROSS):
        mask |= ((centre != 0) & (pad[1 + di:1 + di + h, 1 + dj:1 + dj + w] != centre)).astype(np.uint8) << np.uint8(s)
    mask = mask.ravel()
    cnt = _POPCOUNT[mask]
    first = np.cumsum(cnt, dtype=np.int64) - cnt                 # compact index of a pixel's first edge
    keys = np.flatnonzero((mask[:, None] >> np.arange(4, dtype=np.uint8)) & 1)      # ascending 4 * p + s
    E = len(keys)
    if E == 0:
        return empty_outlines()
    if E >= 2 ** 31:
        raise ValueError(f"polygonize: {E} boundary edges do not fit int32")
    pix, side = keys >> 2, keys & 3
    i, j = pix // w, pix % w
    lab = labels.ravel()[pix]
    bi, bj = i + _AHEAD[side, 0], j + _AHEAD[side, 1]
    ai, aj = i + _AHEAD_LEFT[side, 0], j + _AHEAD_LEFT[side, 1]
    same_b = pad[bi + 1, bj + 1] == lab
    same_a = pad[ai + 1, aj + 1] == lab
    straight = same_b & ~same_a
    left = same_a if connectivity == 8 else same_a & same_b
    q = np.where(left, ai * w + aj, np.where(straight, bi * w + bj, pix))
    t = np.where(left, (side + 3) & 3, np.where(straight, side, (side + 1) & 3))
    succ = first[q] + _POP_LOW[mask[q], t]
    corner = ~straight
    m, d = _jump(succ, corner)

    heads = np.flatnonzero(m == np.arange(E, dtype=np.int32))    # ascending ring id
    total = d[succ[heads]].astype(np.int64) + corner[heads]
    ring_label = lab[heads]
    order = np.argsort(ring_label, kind="stable")                # (label, ring id): the exterior 4 * root is a patch's smallest key
    heads, total, ring_label = heads[order], total[order], ring_label[order]
    R = len(heads)
    ring_offsets = np.concatenate([[0], np.cumsum(total)]).astype(np.int64)
    row_of = np.full(E, -1, np.int64)
    row_of[heads] = np.arange(R)
    ce = np.flatnonzero(corner)
    if len(ce) != ring_offsets[-1]:
        raise ValueError("polygonize: the label plane is not a patch labelling (the successor is no bijection)")
    row = row_of[m[ce]]
    at = ring_offsets[row] + np.where(m[ce] == ce, 0, total[row] - d[ce])
    xy = np.empty((len(ce), 2), np.int32)
    xy[at, 0] = SUBPIXEL * (j[ce] + _END_X[side[ce]])
    xy[at, 1] = SUBPIXEL * (i[ce] + _END_Y[side[ce]])
    new_polygon = np.concatenate([[True], ring_label[1:] != ring_label[:-1]])
    values = classes_u8.ravel()[ring_label[new_polygon].astype(np.int64) - 1]
    return PolygonSet(xy, ring_offsets, np.cumsum(new_polygon) - 1, values)


def _check_connectivity(connectivity, what: str) -> int:
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError(f"{what}: connectivity must be 4 or 8, got {connectivity!r}")
    return int(connectivity)


def polygonize_host(classes_u8, K: int, connectivity: int = 8, labels=None) -> PolygonSet:
    """the outlines of the patches of a uint8 class map [h, w] (module contract) in vectorised numpy: the CPU path and the
    yardstick of the GPU tests.  ``labels``: the map's label plane (``label_patches_host`` with the same connectivity,
    sieved with the map or not) when the caller has it already, else it is computed here.  2 <= K <= 8; sides <= 16384"""
    K = int(K)
    if not 2 <= K <= MAX_CLASSES:
        raise ValueError(f"polygonize: K must be in 2..{MAX_CLASSES}, got {K}")
    connectivity = _check_connectivity(connectivity, "polygonize")
    c = _check_map(classes_u8, "polygonize")
    if max(c.shape) > MAX_SIDE:
        raise ValueError(f"polygonize: raster {c.shape[0]}x{c.shape[1]} must be 1..{MAX_SIDE} in height and width")
    if int(c.max()) >= K:
        raise ValueError(f"polygonize: class value {int(c.max())} out of range (K={K})")
    if labels is None:
        lab = label_patches_host(c, K, connectivity)
    else:
        lab = _check_labels(labels, c.shape, "polygonize")
        if ((lab != 0) != (c != 0)).any() or int(lab.min()) < 0 or int(lab.max()) > c.size:
            raise ValueError("polygonize: labels and classes do not belong together")
    return outlines_from_labels(lab, c, connectivity)


def polygonize(classes, K: int, connectivity: int = 8, device=None) -> PolygonSet:
    """``polygonize_host`` for a host array; on a HIP device (``classes`` a device tensor, or ``device`` a ``cuda`` device:
    the array is uploaded) ``ops.label_patches`` + ``ops.patch_outlines`` — only the four ``PolygonSet`` arrays come back"""
    import torch
    connectivity = _check_connectivity(connectivity, "polygonize")
    dev = classes.device if isinstance(classes, torch.Tensor) else (None if device is None else torch.device(device))
    if dev is not None and dev.type == "cuda":
        from .. import ops
        from .analysis import device_labels, map_plane
        is_tensor = isinstance(classes, torch.Tensor)
        c = classes.to(dev) if is_tensor else map_plane(_check_map(classes, "polygonize"), None, False, dev)
        c, labels, _, err = device_labels(c, K, PatchConfig(connectivity), areas=False)
        polys = ops.patch_outlines(labels, c, connectivity)
        if int(err):
            raise ValueError(f"polygonize: class value out of range (K={K})")
        return polys
    return polygonize_host(classes.numpy() if isinstance(classes, torch.Tensor) else classes, K, connectivity)


# ---------------------------------------------------------------------------------------------- GeoJSON
def outlines_geojson(polys: PolygonSet, transform=None, value_property: str = "type",
                     table: Optional[PatchTable] = None, rfc7946_winding: bool = False, properties=None) -> dict:
    """a GeoJSON ``FeatureCollection`` with one ``Polygon`` feature per polygon: the exterior ring, then the holes, every
    ring closed by repeating its first vertex.  Coordinates are ``x0 + x * dx, y0 + y * dy`` for the north-up GDAL
    geotransform ``(x0, dx, rx, y0, ry, dy)`` (rotation terms other than zero raise ``ValueError``, as in
    ``PolygonSet.to_pixels``); None gives pixel coordinates.  ``properties`` holds the class under ``value_property``, so
    that ``PolygonSet.from_geojson(..., keep_values=None)`` reads it back, and with the ``PatchTable`` of the same label
    plane also ``root``, ``area`` and ``area_m2``.  ``properties``: a mapping from name to a sequence with one entry per
    polygon (a wrong length is a ``ValueError``); every entry goes into its feature's ``properties`` as a Python scalar —
    ``properties={"state": tracks.b_state, "matched": match.b_to_a >= 0}`` colours a change map.

    Vertex order: by default every ring keeps the order of the canonical form, so that ``from_geojson(...).to_pixels(
    transform)`` gives the input arrays back exactly.  The canonical exterior has POSITIVE shoelace area in pixel
    coordinates, where y points down; a north-up transform (dy < 0) mirrors y, so in world coordinates that exterior is
    clockwise (signed area ``dx * dy *`` the pixel area < 0).  ``rfc7946_winding=True`` writes every ring whose world
    orientation is not the one RFC 7946 asks for (exterior counter-clockwise, holes clockwise) backwards from its first
    vertex: the same rings, but a reader gets the reversed vertex order."""
    if not isinstance(polys, PolygonSet):
        raise ValueError(f"outlines_geojson: expected a PolygonSet, got {type(polys).__name__}")
    polys._need_pixels("outlines_geojson")
    if transform is None:
        x0, dx, y0, dy = 0.0, 1.0, 0.0, 1.0
    else:
        t = [float(v) for v in transform]
        if len(t) != 6:
            raise ValueError("outlines_geojson: a GDAL geotransform has six terms (x0, dx, rx, y0, ry, dy)")
        x0, dx, rx, y0, ry, dy = t
        if rx != 0.0 or ry != 0.0:
            raise ValueError("outlines_geojson: rotated geotransforms are not supported (north-up only)")
        if dx == 0.0 or dy == 0.0:
            raise ValueError("outlines_geojson: zero pixel size")
    if table is not None:
        if not isinstance(table, PatchTable) or table.n != len(polys):
            raise ValueError("outlines_geojson: table must be the PatchTable of the outlines' label plane (one row per polygon)")
        area_m2 = table.area_m2()
    extra = {}
    for name, column in (properties or {}).items():
        column = column.tolist() if isinstance(column, np.ndarray) else [v.item() if isinstance(v, np.generic) else v
                                                                         for v in column]
        if len(column) != len(polys):
            raise ValueError(f"outlines_geojson: property {name!r} has {len(column)} entries for {len(polys)} polygons")
        extra[str(name)] = column
    world = np.empty((len(polys.xy), 2), np.float64)
    world[:, 0] = x0 + (polys.xy[:, 0] / SUBPIXEL) * dx
    world[:, 1] = y0 + (polys.xy[:, 1] / SUBPIXEL) * dy
    world = world.tolist()
    ro, rp = polys.ring_offsets.tolist(), polys.ring_polygon
    first_ring = np.searchsorted(rp, np.arange(len(polys) + 1)).tolist()
    # canonical: exterior positive, holes negative in pixel coordinates; the world sign is that times sign(dx * dy)
    reverse = rfc7946_winding and dx * dy < 0
    features = []
    for k in range(len(polys)):
        rings = []
        for r in range(first_ring[k], first_ring[k + 1]):
            ring = world[ro[r]:ro[r + 1]]
            if reverse:
                ring = ring[:1] + ring[:0:-1]
            rings.append(ring + ring[:1])
        props = {value_property: int(polys.values[k])}
        if table is not None:
            props.update(root=int(table.root[k]), area=int(table.area[k]), area_m2=float(area_m2[k]))
        for name, column in extra.items():
            props[name] = column[k]
        features.append({"type": "Feature", "properties": props, "geometry": {"type": "Polygon", "coordinates": rings}})
    return {"type": "FeatureCollection", "features": features}


def write_outlines_geojson(path, polys: PolygonSet, transform=None, value_property: str = "type",
                           table: Optional[PatchTable] = None, rfc7946_winding: bool = False, properties=None) -> None:
    """``outlines_geojson`` written to ``path`` as JSON"""
    obj = outlines_geojson(polys, transform, value_property, table, rfc7946_winding, properties=properties)
    with open(os.fspath(path), "w") as f:
        json.dump(obj, f)
