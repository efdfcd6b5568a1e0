"""Polygon rasterisation on the host (deadtrees_amd/data/polygons.py): the known answers of the contract, ``rasterize_host``
against a slow scalar restatement of the rule written here in plain Python integers (per pixel, per edge, no scanline
shortcut), the supersampling property, the edge cases, the parsers, and the two integrations that run without a device
(``pool_from_rasters(device="cpu")`` and ``Tiler.stats``).  Integers only: every comparison is exact."""
import functools
import json

import numpy as np
import pytest

from polygon_fixtures import KNOWN, packed_polygons, ring_polygon, star_polygons


def _ps(polys):
    from deadtrees_amd.data.polygons import PolygonSet
    return PolygonSet.from_polygons(polys)


def _host(polys, h, w, all_touched=True):
    from deadtrees_amd.data.polygons import PolygonSet, rasterize_host
    return rasterize_host(polys if isinstance(polys, PolygonSet) else _ps(polys), h, w, all_touched)


# ---------------------------------------------------------------------------------------------- the rule, restated
def _q(v):
    import math
    return int(math.floor(float(v) * 256 + 0.5))


def scalar_rule(polys, h, w):
    """(all_touched map, centre-only map) from the contract's words: snapped vertices, every ring closed, edges as they are
    listed (neither upward nor filtered), Python ints"""
    touched = [[0] * w for _ in range(h)]
    centre = [[0] * w for _ in range(h)]
    for poly in polys:
        value, rings = poly[0], [poly[1], *(poly[2] if len(poly) > 2 else [])]
        segs = []
        for ring in rings:
            pts = [(_q(x), _q(y)) for x, y in np.asarray(ring, dtype=np.float64)[:, :2]]
            if pts[0] == pts[-1]:
                pts = pts[:-1]
            segs += [(pts[k], pts[(k + 1) % len(pts)]) for k in range(len(pts))]
        for i in range(h):
            for j in range(w):
                cx, cy = 256 * j + 128, 256 * i + 128
                inside = touch = False
                for (ax, ay), (bx, by) in segs:
                    if (ax, ay) == (bx, by):
                        continue
                    if (ay <= cy) != (by <= cy):
                        cross = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
                        if (cross > 0) == (by > ay) and cross != 0:
                            inside = not inside
                    if (min(ax, bx) < 256 * j + 256 and max(ax, bx) > 256 * j and min(ay, by) < 256 * i + 256
                            and max(ay, by) > 256 * i):
                        c = [(bx - ax) * (py - ay) - (by - ay) * (px - ax)
                             for px in (256 * j, 256 * j + 256) for py in (256 * i, 256 * i + 256)]
                        touch = touch or min(c) < 0 < max(c)
                for plane, burnt in ((touched, inside or touch), (centre, inside)):
                    if burnt and (plane[i][j] == 0 or value < plane[i][j]):
                        plane[i][j] = value
    return np.array(touched, np.uint8).reshape(h, w), np.array(centre, np.uint8).reshape(h, w)


SCALAR_CASES = {
    "stars": (lambda: star_polygons(11, 24, 24, 40), (24, 40)),
    "stars, odd raster": (lambda: star_polygons(12, 16, 19, 33), (19, 33)),
    "packed": (lambda: packed_polygons(23, 60, 12, 20), (12, 20)),
    "ring": (lambda: ring_polygon(5, 240, 20, 30) + star_polygons(6, 3, 20, 30, values=(1, 3)), (20, 30)),
    "one pixel": (lambda: star_polygons(13, 6, 1, 1, radius=(0.2, 0.9)), (1, 1)),
}


@pytest.mark.parametrize("case", list(SCALAR_CASES))
def test_rasterize_host_against_the_scalar_rule(case):
    make, (h, w) = SCALAR_CASES[case]
    polys = make()
    want_touched, want_centre = scalar_rule(polys, h, w)
    assert np.array_equal(_host(polys, h, w, True), want_touched)
    assert np.array_equal(_host(polys, h, w, False), want_centre)
    if h * w > 1:
        assert 0 < np.count_nonzero(want_centre) < np.count_nonzero(want_touched) < h * w       # not vacuous


# ---------------------------------------------------------------------------------------------- known answers
@pytest.mark.parametrize("k", range(len(KNOWN)), ids=[k[0] for k in KNOWN])
def test_known_answers(k):
    name, polys, (h, w), n_touched, n_centre = KNOWN[k]
    touched, centre = _host(polys, h, w, True), _host(polys, h, w, False)
    want_t, want_c = scalar_rule(polys, h, w)
    assert np.array_equal(touched, want_t) and np.array_equal(centre, want_c)
    assert np.count_nonzero(touched) == n_touched
    if n_centre is not None:
        assert np.count_nonzero(centre) == n_centre
    want = np.zeros((h, w), np.uint8)
    if name == "rectangle on the grid":
        want[2:7, 3:9] = 1                           # edges on grid lines burn neither side: both modes
        assert np.array_equal(touched, want) and np.array_equal(centre, want)
    elif name == "rectangle off the grid":
        want[2:7, 3:10] = 1                          # x 3.5 .. 9.01 touches columns 3 and 9
        assert np.array_equal(touched, want)
        want[:] = 0
        want[2:7, 3:9] = 1                           # centres 3.5 .. 8.5: a centre ON the left edge has the crossing of the
                                                     # right edge alone strictly on its ray (cross == 0 is no crossing)
        assert np.array_equal(centre, want)
    elif name == "sliver":
        want[4, 1:11] = 1
        assert np.array_equal(touched, want) and not centre.any()
    else:
        want[2:20, 2:20] = 1
        want[6:16, 6:16] = 0
        assert np.array_equal(touched, want) and np.array_equal(centre, want)


# ---------------------------------------------------------------------------------------------- supersampling
def test_supersampling_property():
    """no pixel that holds an inside sample point (8 x 8 per pixel, matplotlib's point-in-path on the snapped ring) is left
    unburnt; with all_touched=False every burnt pixel's centre is inside"""
    mpath = pytest.importorskip("matplotlib.path")
    rng = np.random.default_rng(3)
    h = w = 32
    sub = (np.arange(8) + 0.5) / 8
    gx, gy = np.meshgrid((np.arange(w)[:, None] + sub[None]).ravel(), (np.arange(h)[:, None] + sub[None]).ravel())
    samples = np.stack([gx.ravel(), gy.ravel()], axis=1)
    centres = np.stack(np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5), axis=-1).reshape(-1, 2)
    burnt = touch_only = 0
    for _ in range(40):
        ang = np.sort(rng.uniform(0, 2 * np.pi, 9))
        ring = np.stack([16 + rng.uniform(2, 14, 9) * np.cos(ang), 16 + rng.uniform(2, 14, 9) * np.sin(ang)], axis=1)
        ring = np.floor(ring * 256 + 0.5) / 256                                    # what the rasteriser sees
        path = mpath.Path(np.concatenate([ring, ring[:1]]), closed=True)
        touched, centre = _host([(1, ring)], h, w, True), _host([(1, ring)], h, w, False)
        inside = path.contains_points(samples).reshape(h * 8, w * 8)
        holds = inside.reshape(h, 8, w, 8).any(axis=(1, 3))
        assert not np.any(holds & (touched == 0))
        # centres strictly inside by a margin are burnt, burnt centres are not outside by a margin (the boundary itself
        # belongs to the half-open rule, not to matplotlib's)
        assert np.all(centre.ravel()[path.contains_points(centres, radius=-1e-6)] == 1)
        assert not np.any(centre.ravel()[~path.contains_points(centres, radius=1e-6)])
        assert np.all(touched[centre == 1] == 1)
        burnt += np.count_nonzero(touched)
        touch_only += np.count_nonzero(touched != centre)
    assert 0 < touch_only < burnt


# ---------------------------------------------------------------------------------------------- edge cases
def test_min_value_merge_in_either_order():
    a, b = (1, [(2, 2), (9, 2), (9, 9), (2, 9)]), (2, [(5, 5), (13, 5), (13, 13), (5, 13)])
    want = np.zeros((16, 16), np.uint8)
    want[5:13, 5:13] = 2
    want[2:9, 2:9] = 1
    assert np.array_equal(_host([a, b], 16, 16), want)
    assert np.array_equal(_host([b, a], 16, 16), want)


def test_holes_are_even_odd_over_all_rings():
    outer, hole, island = [(1, 1), (15, 1), (15, 15), (1, 15)], [(4, 4), (12, 4), (12, 12), (4, 12)], \
        [(6, 6), (10, 6), (10, 10), (6, 10)]
    want = np.zeros((16, 16), np.uint8)
    want[1:15, 1:15] = 3
    want[4:12, 4:12] = 0
    assert np.array_equal(_host([(3, outer, [hole])], 16, 16), want)
    want[6:10, 6:10] = 3                                   # a ring inside the hole is inside again
    assert np.array_equal(_host([(3, outer, [hole, island])], 16, 16), want)


def test_polygon_inside_one_pixel():
    tri = [(1, [(5.2, 3.1), (5.4, 3.15), (5.3, 3.3)])]     # misses the centre (5.5, 3.5)
    want = np.zeros((8, 8), np.uint8)
    want[3, 5] = 1
    assert np.array_equal(_host(tri, 8, 8, True), want)
    assert not _host(tri, 8, 8, False).any()


def test_vertices_outside_the_raster():
    big = [(2, [(-50, -50), (100, -40), (90, 120), (-60, 70)])]
    assert np.all(_host(big, 10, 14) == 2) and np.all(_host(big, 10, 14, False) == 2)
    half = [(1, [(-5, -5), (4, -5), (4, 30), (-5, 30)])]
    want = np.zeros((10, 14), np.uint8)
    want[:, :4] = 1
    assert np.array_equal(_host(half, 10, 14), want)
    away = [(1, [(20, 2), (30, 2), (30, 8)])]
    assert not _host(away, 10, 14).any()


def test_segment_on_a_grid_line_burns_neither_side():
    # a degenerate polygon: all of it on the line y = 4, and one on x = 3
    assert not _host([(1, [(1, 4), (9, 4), (5, 4)])], 8, 12).any()
    assert not _host([(1, [(3, 1), (3, 7), (3, 4)])], 8, 12).any()
    # a thin triangle on the line: only the side it leans to
    got = _host([(1, [(1, 4), (9, 4), (9, 4.2)])], 8, 12)
    want = np.zeros((8, 12), np.uint8)
    want[4, 1:9] = 1
    assert np.array_equal(got, want)


def test_duplicate_vertex_changes_nothing():
    ring = [(1.3, 1.2), (9.7, 2.1), (8.2, 9.6), (2.4, 7.7)]
    twice = [ring[0], ring[1], ring[1], ring[2], ring[2], ring[2], ring[3]]
    for mode in (True, False):
        assert np.array_equal(_host([(1, ring)], 12, 12, mode), _host([(1, twice)], 12, 12, mode))
    closed = ring + [ring[0]]                              # GeoJSON's closing vertex
    assert np.array_equal(_host([(1, ring)], 12, 12), _host([(1, closed)], 12, 12))


def test_snapping_and_to_pixels():
    from deadtrees_amd.data.polygons import PolygonSet, snap, tile_transform
    assert snap([0.0, 1.0, 0.001953125, 0.00195312, -0.001953125, -1.5, 3.998046875]).tolist() == [0, 256, 1, 0, 0, -384, 1024]
    ps = _ps([(2, [(0.5, 0.25), (3, 0.25), (3, 2)])])
    assert ps.xy.dtype == np.int32 and ps.xy.tolist() == [[128, 64], [768, 64], [768, 512]]
    assert ps.bounds.tolist() == [[128, 64, 768, 512]] and ps.values.tolist() == [2] and len(ps) == 1
    assert ps.ring_offsets.tolist() == [0, 3] and ps.ring_polygon.tolist() == [0]
    with pytest.raises(ValueError):
        ps.xy[0, 0] = 1                                    # immutable
    # a 10 m grid, top-left corner at (500000, 5400000): world (500025, 5399980) is column 2.5, row 2.0
    gt = (500000.0, 10.0, 0.0, 5400000.0, 0.0, -10.0)
    world = {"type": "FeatureCollection", "features": [{"type": "Feature", "properties": {"type": 1}, "geometry": {
        "type": "Polygon", "coordinates": [[[500025, 5399980], [500060, 5399980], [500060, 5399915], [500025, 5399980]]]}}]}
    px = PolygonSet.from_geojson(world).to_pixels(gt)
    assert px.xy.tolist() == [[640, 512], [1536, 512], [1536, 2176]]
    assert tile_transform(500000, 500100, 5399900, 5400000, 10, 10) == gt
    assert tile_transform(500000, 500100, 5400000, 5399900, 10, 10) == gt
    with pytest.raises(ValueError):
        PolygonSet.from_geojson(world).to_pixels((500000.0, 10.0, 0.1, 5400000.0, 0.0, -10.0))
    with pytest.raises(ValueError):
        PolygonSet.from_geojson(world).clip_to(10, 10)     # still in world coordinates
    with pytest.raises(ValueError):
        _host(PolygonSet.from_geojson(world), 10, 10)


def test_validation():
    from deadtrees_amd.data.polygons import PolygonSet, rasterize_host
    tri = [(0, 0), (4, 0), (4, 4)]
    for bad in (0, 256, -1, 1.5):
        with pytest.raises(ValueError):
            _ps([(bad, tri)])
    with pytest.raises(ValueError):
        _ps([(1, [(0, 0), (4, 0)])])                       # two vertices
    with pytest.raises(ValueError):
        _ps([(1, [(0, 0), (4, 0), (0, 0)])])               # two vertices and the closing one
    with pytest.raises(ValueError):
        _ps([(1, tri, [[(1, 1), (2, 1)]])])                # a hole of two
    with pytest.raises(ValueError):
        _ps([(1, [(0, 0), (4, 0), (32768.5, 4)])])         # |q| > 2^23
    with pytest.raises(ValueError):
        _ps([(1, [(0, 0), (4, 0), (float("nan"), 4)])])
    assert _ps([(1, [(0, 0), (4, 0), (32768, -32768)])]).xy.max() == 1 << 23
    with pytest.raises(ValueError):
        PolygonSet(np.zeros((3, 2), np.float64), [0, 3], [0], [1])
    with pytest.raises(ValueError):
        PolygonSet(np.zeros((3, 2), np.int32), [0, 3], [1], [1, 1])
    for h, w in ((0, 4), (4, 0), (16385, 4), (4, 16385)):
        with pytest.raises(ValueError):
            rasterize_host(_ps([(1, tri)]), h, w)
    empty = _ps([])
    assert len(empty) == 0 and not rasterize_host(empty, 5, 7).any()


def test_locations_csv_and_clip_to(tmp_path):
    from deadtrees_amd.data.polygons import read_locations_csv, tile_transform
    f = tmp_path / "locations.csv"
    f.write_text("ortho_ms_2019_EPSG3044_000_000.tif;500000.0;500409.6;5399590.4;5400000.0\n"
                 "ortho_ms_2019_EPSG3044_000_001.tif;500409.6;500819.2;5399590.4;5400000.0\n\n")
    loc = read_locations_csv(f)
    assert list(loc) == ["ortho_ms_2019_EPSG3044_000_000.tif", "ortho_ms_2019_EPSG3044_000_001.tif"]
    assert loc["ortho_ms_2019_EPSG3044_000_001.tif"] == (500409.6, 500819.2, 5399590.4, 5400000.0)
    gt = tile_transform(*loc["ortho_ms_2019_EPSG3044_000_001.tif"], 2048, 2048)
    assert gt[0] == 500409.6 and gt[3] == 5400000.0 and gt[2] == gt[4] == 0.0
    assert gt[1] == pytest.approx(0.2) and gt[5] == pytest.approx(-0.2)
    (tmp_path / "bad.csv").write_text("a.tif;1;2;3\n")
    with pytest.raises(ValueError):
        read_locations_csv(tmp_path / "bad.csv")
    (tmp_path / "bad2.csv").write_text("a.tif;1;2;3;x\n")
    with pytest.raises(ValueError):
        read_locations_csv(tmp_path / "bad2.csv")

    inside, across = (1, [(2, 2), (6, 2), (6, 6)]), (2, [(-3, 4), (3, 4), (3, 9), (-3, 9)], [[(-1, 5), (1, 5), (1, 7)]])
    right, on_edge = (3, [(20, 2), (26, 2), (26, 6)]), (1, [(-4, 0), (0, 0), (0, 5)])       # on_edge: maxx == 0 exactly
    ps = _ps([right, inside, on_edge, across])
    kept = ps.clip_to(12, 16)
    assert len(kept) == 2 and kept.values.tolist() == [1, 2] and kept.ring_polygon.tolist() == [0, 1, 1]
    assert kept.ring_offsets.tolist() == [0, 3, 7, 10]
    assert np.array_equal(_host(kept, 12, 16), _host(ps, 12, 16))
    assert len(ps.clip_to(12, 30)) == 3


def test_geojson(tmp_path):
    from deadtrees_amd.data.polygons import PolygonSet
    sq = [[1, 1], [5, 1], [5, 5], [1, 5], [1, 1]]
    hole = [[2, 2], [4, 2], [4, 4], [2, 2]]
    far = [[8, 8], [11, 8], [11, 11], [8, 8]]

    def feat(value, geom_type, coords, name="type"):
        return {"type": "Feature", "properties": {name: value}, "geometry": {"type": geom_type, "coordinates": coords}}

    fc = {"type": "FeatureCollection", "features": [
        feat(2, "Polygon", [sq, hole]), feat("1.0", "MultiPolygon", [[far], [sq]], name="Type"), feat(0, "Polygon", [far]),
        feat(7, "Polygon", [far])]}
    ident = (0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
    ps = PolygonSet.from_geojson(fc).to_pixels(ident)
    assert ps.values.tolist() == [2, 1, 1] and ps.ring_polygon.tolist() == [0, 0, 1, 2]       # exploded; 0 and 7 dropped
    want = _host([(2, sq, [hole]), (1, far), (1, sq)], 12, 12)
    assert np.array_equal(_host(ps, 12, 12), want) and set(np.unique(want)) == {0, 1}
    assert PolygonSet.from_geojson(fc, keep_values=(2, 7)).values.tolist() == [2, 7]
    assert PolygonSet.from_geojson(fc, simple=True).values.tolist() == [1, 1, 1]
    path = tmp_path / "polys.geojson"
    path.write_text(json.dumps(fc))
    for src in (path, str(path), json.dumps(fc)):
        assert np.array_equal(_host(PolygonSet.from_geojson(src).to_pixels(ident), 12, 12), want)
    with pytest.raises(ValueError):                        # value 0 with keep_values=None: outside 1..255
        PolygonSet.from_geojson(fc, keep_values=None)
    with pytest.raises(ValueError):
        PolygonSet.from_geojson({"type": "FeatureCollection", "features": [feat(1, "LineString", sq)]})
    with pytest.raises(ValueError):
        PolygonSet.from_geojson({"type": "FeatureCollection", "features": [feat(1, "Point", [1, 1])]})
    with pytest.raises(ValueError):
        PolygonSet.from_geojson({"type": "Feature"})
    with pytest.raises(ValueError):
        PolygonSet.from_geojson({"type": "FeatureCollection", "features": [feat(1, "Polygon", [sq], name="class")]})
    with pytest.raises(ValueError):
        PolygonSet.from_geojson({"type": "FeatureCollection", "features": [feat("conifer", "Polygon", [sq])]})
    assert PolygonSet.from_geojson({"type": "FeatureCollection", "features": [feat(1, "Polygon", [sq], name="class")]},
                                   value_property="class").values.tolist() == [1]


def test_rasterize_dispatches_to_the_host_without_a_device():
    from deadtrees_amd.data.polygons import rasterize
    ps = _ps(star_polygons(11, 10, 20, 30))
    want = _host(ps, 20, 30)
    got = rasterize(ps, (20, 30))
    assert isinstance(got, np.ndarray) and np.array_equal(got, want)
    assert np.array_equal(rasterize(ps, (20, 30), device="cpu", all_touched=False), _host(ps, 20, 30, False))
    buf = np.full((22, 30), 9, np.uint8)
    assert rasterize(ps, (20, 30), out=buf[1:21]) is not None
    assert np.array_equal(buf[1:21], want) and np.all(buf[0] == 9) and np.all(buf[21] == 9)


# ---------------------------------------------------------------------------------------------- integrations
@functools.lru_cache(maxsize=None)
def _raster_items():
    """two 128 x 128 rasters (one ragged) with polygon masks and land use, and the same with the burnt arrays"""
    rng = np.random.default_rng(17)
    with_polys, with_arrays = [], []
    for n, (h, w) in enumerate(((128, 128), (100, 117))):
        rgbn = rng.integers(0, 256, (4, h, w), dtype=np.uint8)
        rgbn[:, :32, 32:64] = 7                            # one blank sub-tile
        mask = _ps(star_polygons(40 + n, 14, h, w, values=(1, 2), radius=(0.03, 0.1)))
        lu = _ps(star_polygons(50 + n, 5, h, w, values=(1,), radius=(0.3, 0.5)))
        with_polys.append((f"r{n}", rgbn, mask, lu if n == 0 else None))
        with_arrays.append((f"r{n}", rgbn, _host(mask, h, w), _host(lu, h, w) if n == 0 else None))
    return with_polys, with_arrays


def test_pool_from_rasters_on_the_host_with_polygon_maps():
    from deadtrees_amd.data.rasters import pool_from_rasters
    with_polys, with_arrays = _raster_items()
    for select in ("dead", "valid"):
        rec_a, rec_b = {}, {}
        a = pool_from_rasters(with_polys, tile_size=32, source_dim=128, select=select, device="cpu", record=rec_a)
        b = pool_from_rasters(with_arrays, tile_size=32, source_dim=128, select=select, device="cpu", record=rec_b)
        assert a.n == b.n > 0 and a.stats == b.stats and rec_a["table"] == rec_b["table"]
        for x, y in ((a.images, b.images), (a.masks, b.masks), (a.lu, b.lu), (a.sums, b.sums)):
            assert np.array_equal(np.asarray(x), np.asarray(y))
        assert np.asarray(a.masks).any() and 0 < np.count_nonzero(np.asarray(a.lu)) < np.asarray(a.lu).size


def test_tiler_stats_with_polygon_zones():
    from deadtrees_amd.deployment.tiler import Tiler
    h, w = 100, 117
    rng = np.random.default_rng(5)
    zones = _ps(star_polygons(60, 9, h, w, values=(1, 2), radius=(0.15, 0.3)))
    burnt = _host(zones, h, w)
    assert set(np.unique(burnt)) == {0, 1, 2}
    t = Tiler(tile_shape=(128, 128), subtile_shape=(64, 64))
    t.load_array(rng.integers(0, 256, (4, h, w), dtype=np.uint8))
    t.put_batches(rng.integers(0, 3, (len(t.get_batches()), 64, 64), dtype=np.uint8))
    a, b = t.stats(zones=zones, classes=3), t.stats(zones=burnt, classes=3)
    assert a.counts.shape == (3, 3) and np.array_equal(a.counts, b.counts) and int(a.counts.sum()) == h * w
    assert np.array_equal(t.stats(zones=zones, classes=3, n_zones=5).counts, t.stats(zones=burnt, classes=3, n_zones=5).counts)
    with pytest.raises(ValueError):
        t.stats(zones=zones, classes=3, n_zones=2)
    with pytest.raises(ValueError):
        t.stats(zones=_ps([(9, [(1, 1), (5, 1), (5, 5)])]), classes=3)             # more than 8 zones
