"""Dead-tree patch outlines on the host: ``deployment/outlines.py`` — ``polygonize_host`` against a scalar wall follower
written here, hand answers, the properties that tie the outlines to the ``PatchTable`` and to the rasteriser, GeoJSON out
and back, and ``Tiler.stats(..., outlines=True)``.  Integers only: every comparison is exact."""
import functools
import json

import numpy as np
import pytest

from deadtrees_amd.data.polygons import PolygonSet, rasterize_host
from deadtrees_amd.deployment.outlines import (outlines_geojson, polygonize, polygonize_host, write_outlines_geojson)
from deadtrees_amd.deployment.patches import (PatchConfig, label_patches_host, measure_patches_host, patches_host,
                                              sieve_host)

K = 3
CONNECTIVITIES = (4, 8)
FILLS = (0.03, 0.3, 0.59, 0.9)
SHAPES = ((1, 1), (1, 7), (7, 1), (2, 2), (2, 3), (3, 5), (5, 4), (8, 8), (9, 17), (16, 33), (23, 11), (31, 32), (33, 64),
          (40, 70))
TRANSFORM = (60000.0, 0.2, 0, 100000.0, 0, -0.2)

# side s of pixel (i, j): from, to (as offsets to (j, i)); the pixel across it, the pixel B ahead, A = ahead-left (di, dj)
FROM = ((0, 0), (1, 0), (1, 1), (0, 1))
TO = ((1, 0), (1, 1), (0, 1), (0, 0))
ACROSS = ((-1, 0), (0, 1), (1, 0), (0, -1))
AHEAD = ((0, 1), (1, 0), (0, -1), (-1, 0))


def _arrays(p: PolygonSet):
    return p.xy, p.ring_offsets, p.ring_polygon, p.values


def _same(a: PolygonSet, b: PolygonSet):
    for x, y in zip(_arrays(a), _arrays(b)):
        assert x.dtype == y.dtype and np.array_equal(x, y)


# ---------------------------------------------------------------------------------------------- the scalar tracer
def _tracer(classes, labels, connectivity):
    """the contract by walking: owned sides, the successor table, cycles followed edge by edge.  Returns the four
    ``PolygonSet`` arrays as lists and the number of edges"""
    h, w = labels.shape

    def L(i, j):
        return int(labels[i, j]) if 0 <= i < h and 0 <= j < w else 0

    edges = [(i * w + j, s) for i in range(h) for j in range(w) if L(i, j)
             for s in range(4) if L(i + ACROSS[s][0], j + ACROSS[s][1]) != L(i, j)]
    owned = set(edges)

    def succ(p, s):
        i, j = divmod(p, w)
        l = L(i, j)
        bi, bj = i + AHEAD[s][0], j + AHEAD[s][1]
        ai, aj = bi + ACROSS[s][0], bj + ACROSS[s][1]
        if connectivity == 8:
            if L(ai, aj) == l:
                return ai * w + aj, (s + 3) % 4
            if L(bi, bj) == l:
                return bi * w + bj, s
            return p, (s + 1) % 4
        if L(bi, bj) != l:
            return p, (s + 1) % 4
        if L(ai, aj) != l:
            return bi * w + bj, s
        return ai * w + aj, (s + 3) % 4

    image = {e: succ(*e) for e in edges}
    assert set(image.values()) == owned                           # a bijection on the edge set
    rings, seen = [], set()
    for e in edges:                                               # ascending key: the first edge met on a cycle is its id
        if e in seen:
            continue
        ring, cur = [], e
        while cur not in seen:
            seen.add(cur)
            nxt = image[cur]
            if nxt[1] != cur[1]:
                i, j = divmod(cur[0], w)
                ring.append((j + TO[cur[1]][0], i + TO[cur[1]][1]))
            cur = nxt
        assert cur == e
        rings.append((L(*divmod(e[0], w)), 4 * e[0] + e[1], ring))
    rings.sort(key=lambda r: (r[0], r[1]))
    xy, ro, rp, values, last = [], [0], [], [], None
    for label, _, ring in rings:
        if label != last:
            values.append(int(classes.ravel()[label - 1]))
            last = label
        rp.append(len(values) - 1)
        xy += [(256 * x, 256 * y) for x, y in ring]
        ro.append(len(xy))
    return xy, ro, rp, values, len(edges)


def _shoelace2(ring):
    """twice the signed area of a ring of (x, y) rows, exact for integers"""
    x, y = ring[:, 0].astype(object), ring[:, 1].astype(object)
    return int((x * np.roll(y, -1) - np.roll(x, -1) * y).sum())


def _properties(classes, connectivity, polys=None, K=K):
    """what every case must satisfy; returns the outlines"""
    c = np.ascontiguousarray(classes, dtype=np.uint8)
    h, w = c.shape
    labels = label_patches_host(c, K, connectivity)
    table = measure_patches_host(labels, c)
    if polys is None:
        polys = polygonize_host(c, K, connectivity)
    assert polys.xy.dtype == np.int32 and polys.ring_offsets.dtype == np.int64
    assert polys.ring_polygon.dtype == np.int32 and polys.values.dtype == np.uint8
    assert len(polys) == table.n and np.array_equal(polys.values, table.cls)
    areas2 = np.zeros(table.n, object)
    first = np.ones(table.n, bool)
    for r, k in enumerate(polys.ring_polygon):
        a2 = _shoelace2(polys.xy[polys.ring_offsets[r]:polys.ring_offsets[r + 1]])
        assert (a2 > 0) if first[k] else (a2 < 0), (r, k, a2)    # the exterior comes first, holes behind it
        if first[k]:                                              # and starts at the root pixel's top-left corner's edge
            y0, x0 = divmod(int(table.root[k]), w)
            ring = polys.xy[polys.ring_offsets[r]:polys.ring_offsets[r + 1]]
            assert (ring[:, 1].min(), ring[ring[:, 1] == ring[:, 1].min(), 0].min()) == (256 * y0, 256 * x0)
        first[k] = False
        areas2[k] += a2
    assert [int(a) for a in areas2] == [2 * 256 * 256 * int(a) for a in table.area]
    bb = table.bbox.astype(np.int64)
    want = 256 * np.stack([bb[:, 1], bb[:, 0], bb[:, 3] + 1, bb[:, 2] + 1], axis=1) if table.n else np.zeros((0, 4))
    assert np.array_equal(polys.bounds, want)
    assert np.array_equal(rasterize_host(polys, h, w, all_touched=False), c)
    return polys


@functools.lru_cache(maxsize=None)
def _random_map(h, w, fill):
    rng = np.random.default_rng(7919 * h + 31 * w + int(1000 * fill))
    a = np.where(rng.random((h, w)) < fill, rng.integers(1, K, (h, w)), 0).astype(np.uint8)
    a.setflags(write=False)
    return a


# ---------------------------------------------------------------------------------------------- 1. against the tracer
@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_polygonize_host_against_a_scalar_wall_follower(fill, connectivity):
    for h, w in SHAPES:
        c = _random_map(h, w, fill)
        labels = label_patches_host(c, K, connectivity)
        xy, ro, rp, values, _ = _tracer(c, labels, connectivity)
        got = polygonize_host(c, K, connectivity)
        assert np.array_equal(got.xy, np.array(xy, np.int32).reshape(-1, 2)), (h, w)
        assert np.array_equal(got.ring_offsets, ro) and np.array_equal(got.ring_polygon, rp), (h, w)
        assert np.array_equal(got.values, values), (h, w)
        _same(got, polygonize_host(c, K, connectivity, labels=labels))         # the caller's label plane is taken as it is
        _properties(c, connectivity, got)


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_checkerboards_and_full_maps(connectivity):
    yy, xx = np.mgrid[0:13, 0:18]
    for c in (((yy + xx) & 1), 1 + ((yy + xx) & 1), np.ones((13, 18)), np.zeros((13, 18)), (yy == xx), (xx == 17 - yy)):
        c = c.astype(np.uint8)
        labels = label_patches_host(c, K, connectivity)
        xy, ro, rp, values, _ = _tracer(c, labels, connectivity)
        got = _properties(c, connectivity)
        assert np.array_equal(got.xy, np.array(xy, np.int32).reshape(-1, 2))
        assert np.array_equal(got.ring_offsets, ro) and np.array_equal(got.ring_polygon, rp)
        assert np.array_equal(got.values, values)


# ---------------------------------------------------------------------------------------------- 2. hand answers
def _rings(polys):
    """[(polygon, [(x, y), ...] in pixels), ...]"""
    return [(int(polys.ring_polygon[r]), [tuple(v) for v in (polys.xy[polys.ring_offsets[r]:polys.ring_offsets[r + 1]] // 256).tolist()])
            for r in range(len(polys.ring_polygon))]


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_one_pixel(connectivity):
    c = np.zeros((3, 4), np.uint8)
    c[1, 2] = 2
    polys = _properties(c, connectivity)
    assert _rings(polys) == [(0, [(3, 1), (3, 2), (2, 2), (2, 1)])]          # from the top edge on: its end point first
    assert polys.values.tolist() == [2]
    assert np.array_equal(polys.xy, 256 * np.array([(3, 1), (3, 2), (2, 2), (2, 1)]))


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_a_ring_of_ones_has_one_exterior_and_one_hole(connectivity):
    c = np.ones((3, 3), np.uint8)
    c[1, 1] = 0
    polys = _properties(c, connectivity)
    assert _rings(polys) == [(0, [(3, 0), (3, 3), (0, 3), (0, 0)]),
                             (0, [(1, 1), (1, 2), (2, 2), (2, 1)])]            # the hole: id = the bottom side of pixel (0, 1)
    assert polys.values.tolist() == [1]


def test_two_diagonal_pixels():
    c = np.array([[1, 0], [0, 1]], np.uint8)
    eight = _properties(c, 8)
    # one polygon whose exterior passes the shared vertex (1, 1) twice: 8 corners
    assert _rings(eight) == [(0, [(1, 0), (1, 1), (2, 1), (2, 2), (1, 2), (1, 1), (0, 1), (0, 0)])]
    four = _properties(c, 4)
    assert _rings(four) == [(0, [(1, 0), (1, 1), (0, 1), (0, 0)]), (1, [(2, 1), (2, 2), (1, 2), (1, 1)])]
    # the other diagonal
    c = np.array([[0, 1], [1, 0]], np.uint8)
    assert _rings(_properties(c, 8)) == [(0, [(2, 0), (2, 1), (1, 1), (1, 2), (0, 2), (0, 1), (1, 1), (1, 0)])]
    assert len(_properties(c, 4)) == 2


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_a_patch_inside_the_hole_of_another(connectivity):
    c = np.ones((5, 5), np.uint8)
    c[1:4, 1:4] = 0
    c[2, 2] = 2
    polys = _properties(c, connectivity)
    assert _rings(polys) == [(0, [(5, 0), (5, 5), (0, 5), (0, 0)]), (0, [(1, 1), (1, 4), (4, 4), (4, 1)]),
                             (1, [(3, 2), (3, 3), (2, 3), (2, 2)])]
    assert polys.values.tolist() == [1, 2]
    # and filling the hole completely: class 2 touches class 1 along the hole's ring
    c[1:4, 1:4] = 2
    polys = _properties(c, connectivity)
    assert _rings(polys)[1:] == [(0, [(1, 1), (1, 4), (4, 4), (4, 1)]), (1, [(4, 1), (4, 4), (1, 4), (1, 1)])]


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_a_patch_touching_all_four_raster_edges(connectivity):
    c = np.zeros((4, 5), np.uint8)
    c[1, :] = 1
    c[:, 2] = 1                                                   # a cross: 12 corners
    polys = _properties(c, connectivity)
    assert _rings(polys) == [(0, [(3, 0), (3, 1), (5, 1), (5, 2), (3, 2), (3, 4), (2, 4), (2, 2), (0, 2), (0, 1), (2, 1),
                                  (2, 0)])]
    full = _properties(np.full((2, 3), 2, np.uint8), connectivity)
    assert _rings(full) == [(0, [(3, 0), (3, 2), (0, 2), (0, 0)])] and full.values.tolist() == [2]


def test_no_patch_gives_the_empty_set_and_argument_errors():
    empty = polygonize_host(np.zeros((4, 6), np.uint8), K)
    assert len(empty) == 0 and len(empty.xy) == 0 and empty.ring_offsets.tolist() == [0] and len(empty.ring_polygon) == 0
    c = _random_map(9, 17, 0.3)
    for bad in (dict(K=1), dict(K=9), dict(K=2), dict(connectivity=6), dict(connectivity=True)):
        with pytest.raises(ValueError):
            polygonize_host(c, **{"K": K, **bad})
    with pytest.raises(ValueError):
        polygonize_host(c.astype(np.int32), K)
    with pytest.raises(ValueError):
        polygonize_host(c.ravel(), K)
    with pytest.raises(ValueError):
        polygonize_host(c, K, labels=label_patches_host(c, K)[:, :-1])
    with pytest.raises(ValueError):
        polygonize_host(c, K, labels=label_patches_host(c, K).astype(np.int64))
    with pytest.raises(ValueError):
        polygonize_host(c, K, labels=np.zeros(c.shape, np.int32))               # a label plane of another map
    _same(polygonize(c, K, 4), polygonize_host(c, K, 4))                          # no device: the host path
    import torch
    _same(polygonize(torch.from_numpy(c.copy()), K), polygonize_host(c, K))


# ---------------------------------------------------------------------------------------------- 3. the sieve
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_a_sieved_map_gives_the_outlines_of_the_sieved_map(connectivity):
    c = _random_map(40, 70, 0.3)
    labels = label_patches_host(c, K, connectivity)
    sc, sl = sieve_host(c, labels, 4)
    assert not np.array_equal(sc, c)
    got = polygonize_host(sc, K, connectivity, labels=sl)          # the sieved label plane keeps the survivors' labels
    _same(got, polygonize_host(sc, K, connectivity))
    table = measure_patches_host(sl, sc)
    assert len(got) == table.n and int(table.area.min()) >= 4
    _properties(sc, connectivity, got)


# ---------------------------------------------------------------------------------------------- 4. GeoJSON
def _world_area2(ring):
    r = np.array(ring, np.float64)
    x, y = r[:-1, 0] - r[0, 0], r[:-1, 1] - r[0, 1]                # closed: the last vertex repeats the first
    return float((x * np.roll(y, -1) - np.roll(x, -1) * y).sum())


def test_geojson_round_trip_closed_rings_and_properties(tmp_path):
    c = _random_map(33, 64, 0.59)
    polys = polygonize_host(c, K)
    assert len(polys.ring_polygon) > len(polys) > 5               # some holes
    obj = outlines_geojson(polys, TRANSFORM)
    assert obj["type"] == "FeatureCollection" and len(obj["features"]) == len(polys)
    back = PolygonSet.from_geojson(json.dumps(obj), keep_values=None).to_pixels(TRANSFORM)
    _same(back, polys)
    r = 0
    for k, feat in enumerate(obj["features"]):
        assert feat["type"] == "Feature" and feat["geometry"]["type"] == "Polygon"
        assert feat["properties"] == {"type": int(polys.values[k])}
        for n, ring in enumerate(feat["geometry"]["coordinates"]):
            assert ring[0] == ring[-1] and len(ring) == polys.ring_offsets[r + 1] - polys.ring_offsets[r] + 1
            # the canonical exterior is positive in pixel coordinates (y down); the north-up transform mirrors y
            assert (_world_area2(ring) < 0) == (n == 0)
            r += 1
    assert r == len(polys.ring_polygon)
    # pixel coordinates without a transform; another property name
    plain = outlines_geojson(polys, value_property="cls")
    assert plain["features"][0]["properties"] == {"cls": int(polys.values[0])}
    _same(PolygonSet.from_geojson(plain, value_property="cls", keep_values=None).to_pixels((0, 1, 0, 0, 0, 1)), polys)
    assert plain["features"][0]["geometry"]["coordinates"][0][0] == (polys.xy[0] / 256).tolist()
    # with the table
    table = measure_patches_host(label_patches_host(c, K), c)
    rich = outlines_geojson(polys, TRANSFORM, table=table)
    for k, feat in enumerate(rich["features"]):
        assert feat["properties"] == {"type": int(table.cls[k]), "root": int(table.root[k]), "area": int(table.area[k]),
                                      "area_m2": float(table.area_m2()[k])}
    with pytest.raises(ValueError):
        outlines_geojson(polys, TRANSFORM, table=measure_patches_host(label_patches_host(c, K, 4), c))
    # written and read as a file
    path = tmp_path / "outlines.geojson"
    write_outlines_geojson(path, polys, TRANSFORM, table=table)
    _same(PolygonSet.from_geojson(path, keep_values=None).to_pixels(TRANSFORM), polys)
    assert json.loads(path.read_text()) == json.loads(json.dumps(rich))


def test_geojson_exterior_counter_clockwise_in_world_coordinates():
    """RFC 7946 asks for counter-clockwise exteriors and clockwise holes.  The canonical rings cannot have that under a
    north-up transform AND come back vertex for vertex: positive area with y down is negative area with y up.
    ``rfc7946_winding=True`` writes the rings in the RFC's order; read back they are the canonical rings reversed"""
    c = _random_map(33, 64, 0.59)
    polys = polygonize_host(c, K)
    obj = outlines_geojson(polys, TRANSFORM, rfc7946_winding=True)
    for feat in obj["features"]:
        for n, ring in enumerate(feat["geometry"]["coordinates"]):
            assert ring[0] == ring[-1]
            assert (_world_area2(ring) > 0) == (n == 0)           # the exterior ring has positive signed area in world coordinates
    back = PolygonSet.from_geojson(obj, keep_values=None).to_pixels(TRANSFORM)
    assert np.array_equal(back.ring_offsets, polys.ring_offsets) and np.array_equal(back.values, polys.values)
    for r in range(len(polys.ring_polygon)):
        a, b = polys.ring_offsets[r], polys.ring_offsets[r + 1]
        assert np.array_equal(back.xy[a:b], np.concatenate([polys.xy[a:a + 1], polys.xy[a + 1:b][::-1]]))
    assert np.array_equal(rasterize_host(back, 33, 64, all_touched=False), c)
    # in pixel coordinates (dx * dy > 0) the canonical order is the RFC's already
    assert outlines_geojson(polys, rfc7946_winding=True) == outlines_geojson(polys)


def test_geojson_rotation_raises_and_an_empty_set_gives_an_empty_collection():
    polys = polygonize_host(_random_map(9, 17, 0.3), K)
    for bad in ((0, 1, 0.1, 0, 0, -1), (0, 1, 0, 0, 0.1, -1), (0, 0, 0, 0, 0, -1), (0, 1, 0, 0, 0), ):
        with pytest.raises(ValueError):
            outlines_geojson(polys, bad)
    with pytest.raises(ValueError):
        outlines_geojson([("not", "a set")])
    empty = polygonize_host(np.zeros((4, 6), np.uint8), K)
    assert outlines_geojson(empty, TRANSFORM) == {"type": "FeatureCollection", "features": []}
    assert len(PolygonSet.from_geojson(outlines_geojson(empty), keep_values=None)) == 0


def test_reexports():
    import deadtrees.deployment.tiler as ref
    from deadtrees_amd.deployment import outlines
    for name in ("polygonize", "polygonize_host", "outlines_geojson", "write_outlines_geojson"):
        assert getattr(ref, name) is getattr(outlines, name)


# ---------------------------------------------------------------------------------------------- 5. Tiler.stats
def test_tiler_stats_with_outlines_and_the_value_errors():
    from deadtrees_amd.deployment.stats import RasterStats
    from deadtrees_amd.deployment.tiler import Tiler, infer_rasters, infer_tile
    c = _random_map(40, 70, 0.3)

    def tiler():
        t = Tiler(tile_shape=(64, 128), subtile_shape=(32, 32))
        t.load_array(np.zeros((4, 40, 70), np.uint8))
        t._outdata[:40, :70] = c
        return t

    before = tiler().stats(classes=K, patches=True)
    assert before.outlines is None and "outlines" not in repr(before)
    for config in (True, PatchConfig(4), PatchConfig(8, 4)):
        t = tiler()
        st = t.stats(classes=K, patches=config, outlines=True)
        cfg = PatchConfig() if config is True else config
        want_c, want_table = patches_host(c, K, cfg)
        assert np.array_equal(t.result, want_c) and st.patches == want_table
        _same(st.outlines, polygonize_host(want_c, K, cfg.connectivity))
        assert len(st.outlines) == st.patches.n
        plain = tiler().stats(classes=K, patches=config)
        assert plain.patches == st.patches and np.array_equal(plain.counts, st.counts) and plain.outlines is None
        assert st != plain and st == st and "outlines=PolygonSet(" in repr(st)
        assert (st + st).outlines is None and (st + st).patches is None
    with pytest.raises(ValueError):
        tiler().stats(classes=K, outlines=True)                   # outlines without patches
    with pytest.raises(ValueError):
        tiler().stats(classes=K, patches=True, outlines="yes")
    with pytest.raises(ValueError):
        RasterStats([[3, 1]], outlines="no set")
    with pytest.raises(ValueError):
        RasterStats([[3, 1]], outlines=before.patches)
    raster = np.zeros((4, 40, 70), np.uint8)
    with pytest.raises(ValueError):
        infer_tile(None, raster, stats=True, outlines=True)
    with pytest.raises(ValueError):
        infer_tile(None, raster, patches=True, outlines=True)
    with pytest.raises(ValueError):
        next(infer_rasters(None, [raster], stats=True, outlines=True))
