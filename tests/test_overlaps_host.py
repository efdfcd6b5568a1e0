"""Patch overlaps on the host (``deployment/overlaps.py``): ``overlap_pairs_host`` against a scalar restatement of the
contract (a Python loop over the pixels that fills a dict) and hand-computed answers; ``PatchOverlaps`` with ``match`` and
``track`` on hand-drawn maps; every ``ValueError``; ``RasterStats(overlaps=...)``; ``outlines_geojson(properties=...)``;
``Tiler.stats(against=...)``.  No GPU."""
import json
import math

import numpy as np
import pytest

from deadtrees_amd.data.polygons import PolygonSet, rasterize_host
from deadtrees_amd.deployment import overlaps as ov
from deadtrees_amd.deployment.outlines import outlines_geojson, polygonize_host, write_outlines_geojson
from deadtrees_amd.deployment.overlaps import PatchOverlaps, overlap_pairs_host, patch_overlaps
from deadtrees_amd.deployment.patches import PatchConfig, label_patches_host, labelled_patches_host
from deadtrees_amd.deployment.stats import PIXEL_AREA_M2, RasterStats
from deadtrees_amd.deployment.tiler import Tiler, infer_rasters, infer_tile, make_blocks_vectorized

K = 3


def _scalar_pairs(la, lb):
    """the contract, pixel by pixel"""
    table = {}
    h, w = la.shape
    for y in range(h):
        for x in range(w):
            if la[y, x] != 0 and lb[y, x] != 0:
                key = (int(la[y, x]) - 1, int(lb[y, x]) - 1)
                table[key] = table.get(key, 0) + 1
    rows = sorted(table)
    return ([a for a, _ in rows], [b for _, b in rows], [table[r] for r in rows])


def _rows(got):
    assert all(v.dtype == np.int64 and v.ndim == 1 for v in got)
    return tuple(v.tolist() for v in got)


def _pairs(a, b, conn_a=8, conn_b=8):
    la = label_patches_host(np.asarray(a, np.uint8), K, conn_a)
    lb = label_patches_host(np.asarray(b, np.uint8), K, conn_b)
    got = _rows(overlap_pairs_host(la, lb))
    assert got == _scalar_pairs(la, lb)
    return got


def _blobs(h, w, seed, density=0.08):
    rng = np.random.default_rng(seed)
    seeds = np.pad(rng.random((h, w)) < density, 1)
    grown = np.zeros((h, w), bool)
    for dy in range(3):
        for dx in range(3):
            grown |= seeds[dy:dy + h, dx:dx + w]
    return (grown * rng.integers(1, 3, (h, w))).astype(np.uint8)


# ---------------------------------------------------------------------------------------------- 1. the table
def test_a_disconnected_intersection_is_one_row():
    a = np.zeros((6, 7), np.uint8)
    a[1:5, 1] = a[1:5, 5] = a[4, 1:6] = 1              # a U: arms in columns 1 and 5, joined along row 4
    b = np.zeros((6, 7), np.uint8)
    b[2, :] = 1                                        # a bar across both arms
    assert _pairs(a, b) == ([1 * 7 + 1], [2 * 7], [2])
    assert _pairs(b, a) == ([2 * 7], [1 * 7 + 1], [2])


def test_touching_patches_of_two_classes_are_two_rows():
    a = np.zeros((3, 6), np.uint8)
    a[1, 1:3] = 1
    a[1, 3:5] = 2
    b = np.ones((3, 6), np.uint8)
    assert _pairs(a, b) == ([7, 9], [0, 0], [2, 2])
    assert _pairs(b, a) == ([0, 0], [7, 9], [2, 2])


def test_a_map_against_itself():
    a = _blobs(40, 50, 0)
    _, labels, table = labelled_patches_host(a, K, PatchConfig())
    got = overlap_pairs_host(labels, labels)
    assert np.array_equal(got[0], table.root) and np.array_equal(got[1], table.root) and np.array_equal(got[2], table.area)
    assert _rows(got) == _scalar_pairs(labels, labels)


def test_random_maps_against_the_scalar_loop():
    for seed in (1, 2, 3):
        a, b = _blobs(37, 53, seed), np.roll(_blobs(37, 53, seed + 20), (1, 2), (0, 1))
        got = _pairs(a, b, 4, 8)
        assert len(got[0]) > 5


def test_roots_above_two_to_the_sixteen_sort_by_a_then_b():
    a = np.zeros((300, 300), np.uint8)
    b = np.zeros((300, 300), np.uint8)
    a[1, 1:4] = 1
    a[297:299, 10:20] = 1
    a[297:300, 200:203] = 2
    b[1, 2:6] = 2
    b[296:300, 15:18] = 1
    b[299, 190:260] = 1
    b[290:298, 201] = 2
    la, lb = label_patches_host(a, K), label_patches_host(b, K)
    got = _rows(overlap_pairs_host(la, lb))
    assert got == ([301, 297 * 300 + 10, 297 * 300 + 200, 297 * 300 + 200],
                   [302, 296 * 300 + 15, 290 * 300 + 201, 299 * 300 + 190], [2, 6, 1, 3])
    assert got == _scalar_pairs(la, lb) and max(got[0]) > 2 ** 16


def test_no_overlap_and_no_patch():
    a = np.zeros((5, 6), np.uint8)
    a[0, 0:2] = 1
    b = np.zeros((5, 6), np.uint8)
    b[3, 3:6] = 2
    zero = np.zeros((5, 6), np.uint8)
    assert _pairs(a, b) == ([], [], []) and _pairs(zero, zero) == ([], [], [])
    apart = patch_overlaps(a, b, K)
    assert len(apart) == 0 and apart.table_a.n == 1 and apart.table_b.n == 1
    m = apart.match()
    assert (m.tp, m.fn, m.fp) == (0, 1, 1) and m.recall == 0.0 and m.precision == 0.0 and m.f1 == 0.0
    assert m.a_to_b.tolist() == [-1] and m.b_to_a.tolist() == [-1] and math.isnan(m.iou[0])
    t = apart.track()
    assert t.a_state.tolist() == [ov.VANISHED] and t.b_state.tolist() == [ov.NEW] and t.growth.tolist() == [0]
    assert t.new_area_m2() == 3 * PIXEL_AREA_M2
    assert apart.covered_a().tolist() == [0] and apart.partners_b().tolist() == [0] and len(apart.iou()) == 0
    nothing = patch_overlaps(zero, zero, K)
    m = nothing.match()
    assert (m.tp, m.fn, m.fp) == (0, 0, 0) and all(math.isnan(v) for v in (m.recall, m.precision, m.f1))
    assert m.per_class(K).tolist() == [[0, 0, 0], [0, 0, 0]]
    t = nothing.track()
    assert len(t.a_state) == 0 and len(t.b_state) == 0 and t.new_area_m2() == 0.0
    assert t.counts() == {"a": dict.fromkeys(ov.A_STATES, 0), "b": dict.fromkeys(ov.B_STATES, 0)}
    one_sided = patch_overlaps(a, zero, K).match()
    assert one_sided.recall == 0.0 and math.isnan(one_sided.precision) and one_sided.f1 == 0.0


# ---------------------------------------------------------------------------------------------- 2. PatchOverlaps
def test_fields_of_patch_overlaps():
    a = np.zeros((4, 8), np.uint8)
    a[0, 0:5] = 1                                      # area 5
    a[2:4, 6:8] = 2                                    # area 4, no partner
    b = np.zeros((4, 8), np.uint8)
    b[0, 0:2] = 1                                      # area 2, inside a's first
    b[0:2, 4] = 2                                      # area 2, one pixel on it
    o = patch_overlaps(a, b, K)
    assert len(o) == 2 and o.a.tolist() == [0, 0] and o.b.tolist() == [0, 4] and o.n.tolist() == [2, 1]
    assert o.ia.tolist() == [0, 0] and o.ib.tolist() == [0, 1] and o.inter is o.n
    assert o.ia.dtype == np.int64 and o.ib.dtype == np.int64
    assert o.union().tolist() == [5, 6] and o.union().dtype == np.int64
    assert o.iou().tolist() == [2 / 5, 1 / 6] and o.iou().dtype == np.float64
    assert o.covered_a().tolist() == [3, 0] and o.covered_b().tolist() == [2, 1] and o.covered_a().dtype == np.int64
    assert o.partners_a().tolist() == [2, 0] and o.partners_a(same_class=True).tolist() == [1, 0]
    assert o.partners_b().tolist() == [1, 1] and o.partners_b(same_class=True).tolist() == [1, 0]
    assert o == patch_overlaps(a, b, K) and o != patch_overlaps(b, a, K) and o != patch_overlaps(a, a, K)
    assert "pairs=2" in repr(o) and "n_a=2" in repr(o)
    for v in (o.a, o.b, o.n, o.ia, o.ib):
        with pytest.raises(ValueError):
            v[0] = 7                                   # read-only
    sieved = patch_overlaps(a, b, K, PatchConfig(8, 5), PatchConfig(4, 2))
    assert sieved.table_a.n == 1 and sieved.table_b.n == 2 and len(sieved) == 2
    assert len(patch_overlaps(a, b, K, PatchConfig(8, 6))) == 0


def test_patch_overlaps_errors():
    a = np.zeros((4, 8), np.uint8)
    a[0, 0:5] = 1
    a[2, 0:3] = 1
    ta = labelled_patches_host(a, K, PatchConfig())[2]
    other = labelled_patches_host(np.ones((4, 9), np.uint8), K, PatchConfig())[2]
    PatchOverlaps(ta, ta, [0, 16], [0, 16], [5, 3])
    for rows in (([0, 7], [0, 16], [5, 3]),            # a root its table does not have
                 ([0, 16], [0, 17], [5, 3]),
                 ([16, 0], [16, 0], [3, 5]),           # not ascending
                 ([0, 0], [16, 16], [1, 1]),           # not strictly
                 ([0, 0], [16, 0], [1, 1]),
                 ([0, 16], [0, 16], [0, 3]),           # n below 1
                 ([0, 16], [0, 16], [5, 4]),           # n above the smaller area
                 ([0, 16], [0, 16], [5]),
                 ([[0, 16]], [[0, 16]], [[5, 3]])):
        with pytest.raises(ValueError):
            PatchOverlaps(ta, ta, *rows)
    with pytest.raises(ValueError):
        PatchOverlaps(ta, other, [], [], [])
    with pytest.raises(ValueError):
        PatchOverlaps(ta, None, [], [], [])
    la = label_patches_host(a, K)
    for bad in ((la.astype(np.int64), la), (la, la.astype(np.uint8)), (la, la[:, :-1]), (la[:0], la[:0]),
                (la.ravel(), la.ravel())):
        with pytest.raises(ValueError):
            overlap_pairs_host(*bad)
    o = PatchOverlaps(ta, ta, [0, 16], [0, 16], [5, 3])
    for bad in (0, 0.0, -0.5, 1.5, True):
        with pytest.raises(ValueError):
            o.match(min_iou=bad)
    with pytest.raises(ValueError):
        o.match().per_class(1)
    polys = PolygonSet.from_polygons([(3, [(1, 1), (4, 1), (4, 3), (1, 3)])])
    with pytest.raises(ValueError):
        patch_overlaps(polys, a, K)                     # a polygon value >= K
    for bad in (dict(K=1), dict(K=9), dict(config_a=True), dict(config_b=8)):
        with pytest.raises(ValueError):
            patch_overlaps(a, a, **{"K": K, **bad})
    with pytest.raises(ValueError):
        patch_overlaps(a, a[:, :-1], K)
    with pytest.raises(ValueError):
        patch_overlaps(a, a.astype(np.int32), K)
    with pytest.raises(ValueError):
        patch_overlaps(a + 3, a, K)
    with pytest.raises(ValueError):
        patch_overlaps(polys.select([False]), polys.select([False]), K)      # two polygon sets and no shape


# ---------------------------------------------------------------------------------------------- 3. match
def test_an_iou_of_exactly_one_half():
    a = np.zeros((1, 5), np.uint8)
    b = np.zeros((1, 5), np.uint8)
    a[0, 0:3] = 1
    b[0, 1:4] = 1                                      # inter 2, union 4
    o = patch_overlaps(a, b, K)
    assert o.iou().tolist() == [0.5]
    m = o.match(0.5)
    assert (m.tp, m.fn, m.fp) == (1, 0, 0) and m.a_to_b.tolist() == [0] and m.b_to_a.tolist() == [0]
    assert m.iou.tolist() == [0.5] and m.recall == 1.0 and m.precision == 1.0 and m.f1 == 1.0
    m = o.match(0.51)
    assert (m.tp, m.fn, m.fp) == (0, 1, 1) and m.a_to_b.tolist() == [-1]
    assert o.match().tp == 1                           # the default is 0.5
    assert o.match(1 / 3).tp == 1 and o.match(1.0).tp == 0
    assert patch_overlaps(a, a, K).match(1.0).tp == 1


def test_same_class_on_a_conifer_under_a_broadleaf():
    a = np.zeros((4, 6), np.uint8)
    b = np.zeros((4, 6), np.uint8)
    a[1:3, 1:4] = 1
    b[1:3, 1:4] = 2
    a[0, 5] = b[0, 5] = 2                              # and one pair that agrees
    o = patch_overlaps(a, b, K)
    assert o.iou().tolist() == [1.0, 1.0]
    strict, loose = o.match(same_class=True), o.match(same_class=False)
    assert (strict.tp, strict.fn, strict.fp) == (1, 1, 1) and strict.a_to_b.tolist() == [0, -1]
    assert (loose.tp, loose.fn, loose.fp) == (2, 0, 0) and loose.a_to_b.tolist() == [0, 1]
    assert strict.per_class(K).tolist() == [[0, 1, 0], [1, 0, 1]]
    assert loose.per_class(K).tolist() == [[1, 0, 0], [1, 0, 0]]
    assert strict.per_class(4).shape == (3, 3) and strict.per_class(K).dtype == np.int64
    assert strict.recall == 0.5 and strict.precision == 0.5 and strict.f1 == 0.5
    assert o.track().counts()["a"]["CONTINUED"] == 2
    t = o.track(same_class=True)
    assert t.a_state.tolist() == [ov.CONTINUED, ov.VANISHED] and t.b_state.tolist() == [ov.CONTINUED, ov.NEW]


def test_the_greedy_tie_rule_below_one_half():
    a = np.zeros((3, 5), np.uint8)
    b = np.zeros((3, 5), np.uint8)
    a[0, :] = 1                                        # area 5
    b[0, 0:2] = 1                                      # 2 / 5 ...
    b[0, 3:5] = 1                                      # ... and 2 / 5: a tie, the lower row wins
    a[2, 3:5] = 1                                      # a second crown
    b[2, 0:5] = 1                                      # 2 / 5 again
    o = patch_overlaps(a, b, K)
    assert o.iou().tolist() == [0.4, 0.4, 0.4]
    m = o.match(0.25)
    assert m.a_to_b.tolist() == [0, 2] and m.b_to_a.tolist() == [0, -1, 1] and (m.tp, m.fn, m.fp) == (2, 0, 1)
    assert o.match(0.4).tp == 2 and o.match(0.41).tp == 0
    # a better pair goes first, whatever its place in the table
    a = np.zeros((1, 7), np.uint8)
    b = np.zeros((1, 7), np.uint8)
    a[0, :] = 1                                        # area 7
    b[0, 0:2] = 1                                      # 2 / 7, a candidate at 0.25, first in the table
    b[0, 3:7] = 1                                      # 4 / 7
    o = patch_overlaps(a, b, K)
    assert o.iou().tolist() == [2 / 7, 4 / 7]
    m = o.match(0.25)
    assert m.a_to_b.tolist() == [1] and m.b_to_a.tolist() == [-1, 0] and m.iou.tolist() == [4 / 7]
    assert (m.tp, m.fn, m.fp) == (1, 0, 1)


# ---------------------------------------------------------------------------------------------- 4. track
def _two_years():
    a = np.zeros((9, 12), np.uint8)
    b = np.zeros((9, 12), np.uint8)
    a[0, 0:3] = 1                                      # vanished
    b[0, 8:11] = 1                                     # new
    a[2, 0:4] = 1                                      # continued, and grew by one pixel
    b[2, 1:6] = 1
    a[4, 0:8] = 1                                      # split into two
    b[4, 0:3] = b[4, 5:8] = 1
    a[6, 0:3] = a[6, 5:8] = 1                          # two merged into one
    b[6, 0:8] = 1
    a[8, 0:5] = a[8, 7:11] = 1                         # both at once: a5 is split (b5, b6) and b6 merged (a5, a6)
    b[8, 0:2] = b[8, 3:9] = 1
    return a, b


def test_every_state_of_a_hand_drawn_pair_of_years():
    a, b = _two_years()
    o = patch_overlaps(a, b, K)
    assert o.table_a.n == 7 and o.table_b.n == 7 and len(o) == 8
    t = o.track()
    V, C, S, MI = ov.VANISHED, ov.CONTINUED, ov.SPLIT, ov.MERGED_INTO
    N, M, SF = ov.NEW, ov.MERGED, ov.SPLIT_FROM
    assert (V, C, S, MI, N, M, SF) == (0, 1, 2, 3, 0, 2, 3)
    assert t.a_state.dtype == np.uint8 and t.b_state.dtype == np.uint8 and t.growth.dtype == np.int64
    assert t.a_state.tolist() == [V, C, S, MI, MI, S, MI]      # a5: SPLIT goes before MERGED_INTO
    assert t.b_state.tolist() == [N, C, SF, SF, M, SF, M]      # b6: MERGED goes before SPLIT_FROM
    assert t.growth.tolist() == [0, 1, 0, 0, 0, 0, 0]
    assert t.counts() == {"a": {"VANISHED": 1, "CONTINUED": 1, "SPLIT": 2, "MERGED_INTO": 3},
                          "b": {"NEW": 1, "CONTINUED": 1, "MERGED": 2, "SPLIT_FROM": 3}}
    assert t.new_area_m2() == 3 * PIXEL_AREA_M2 and t.new_area_m2(2.0) == 6.0
    assert o.partners_a().tolist() == [0, 1, 2, 1, 1, 2, 1] and o.partners_b().tolist() == [0, 1, 1, 1, 2, 1, 2]
    back = patch_overlaps(b, a, K).track()                      # the years swapped: the states mirror
    assert back.a_state.tolist() == [V, C, MI, MI, S, MI, S] and back.b_state.tolist() == [N, C, M, SF, SF, M, SF]
    assert back.growth.tolist() == [0, -1, 0, 0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------- 5. RasterStats
def test_raster_stats_carry_overlaps_like_outlines():
    a, b = _two_years()
    o = patch_overlaps(a, b, K)
    counts = [[int((b == c).sum()) for c in range(K)]]
    plain = RasterStats(counts, patches=o.table_b)
    st = RasterStats(counts, patches=o.table_b, overlaps=o)
    assert st.overlaps is o and plain.overlaps is None and RasterStats(counts).overlaps is None
    assert "overlaps=PatchOverlaps(pairs=8" in repr(st) and "overlaps" not in repr(plain)
    assert st == RasterStats(counts, patches=o.table_b, overlaps=patch_overlaps(a, b, K))
    assert st != plain and plain != st and plain == RasterStats(counts, patches=o.table_b)
    assert st != RasterStats(counts, patches=o.table_b, overlaps=patch_overlaps(b, b, K))
    total = st + st
    assert total.overlaps is None and total.patches is None and total == RasterStats(2 * np.array(counts))
    for bad in (dict(overlaps=o), dict(patches=o.table_a, overlaps=o), dict(patches=o.table_b, overlaps="yes")):
        with pytest.raises(ValueError):
            RasterStats(counts, **bad)


# ---------------------------------------------------------------------------------------------- 6. GeoJSON properties
def test_outlines_geojson_properties(tmp_path):
    a, b = _two_years()
    o = patch_overlaps(a, b, K)
    polys = polygonize_host(b, K)
    t, m = o.track(), o.match()
    before = outlines_geojson(polys, table=o.table_b)
    assert [sorted(f["properties"]) for f in before["features"]] == [["area", "area_m2", "root", "type"]] * 7
    assert json.dumps(outlines_geojson(polys, table=o.table_b, properties=None)) == json.dumps(before)
    assert json.dumps(outlines_geojson(polys, table=o.table_b, properties={})) == json.dumps(before)
    assert [sorted(f["properties"]) for f in outlines_geojson(polys)["features"]] == [["type"]] * 7
    props = {"state": t.b_state, "matched": m.b_to_a >= 0, "growth": t.growth, "name": [f"p{k}" for k in range(7)],
             "share": [np.float64(0.5)] * 7}
    got = outlines_geojson(polys, table=o.table_b, properties=props)
    text = json.dumps(got)                             # numpy scalars would not serialise
    assert json.loads(text) == got
    for k, (f, f0) in enumerate(zip(got["features"], before["features"])):
        p = f["properties"]
        assert f["geometry"] == f0["geometry"] and {n: p[n] for n in f0["properties"]} == f0["properties"]
        assert p["state"] == int(t.b_state[k]) and type(p["state"]) is int
        assert p["matched"] is bool(m.b_to_a[k] >= 0) and p["growth"] == int(t.growth[k]) and p["name"] == f"p{k}"
        assert type(p["share"]) is float
    path = tmp_path / "change.geojson"
    write_outlines_geojson(path, polys, table=o.table_b, properties=props)
    assert json.loads(path.read_text()) == got
    again = PolygonSet.from_geojson(str(path), keep_values=None).to_pixels((0, 1, 0, 0, 0, 1))
    assert np.array_equal(again.xy, polys.xy) and np.array_equal(again.values, polys.values)
    for bad in ({"state": t.b_state[:-1]}, {"state": list(range(8))}, {"state": t.a_state[:0]}):
        with pytest.raises(ValueError):
            outlines_geojson(polys, properties=bad)


# ---------------------------------------------------------------------------------------------- 7. Tiler.stats, arguments
def _tiler_with(result):
    h, w = result.shape
    t = Tiler(tile_shape=(64, 64), subtile_shape=(32, 32))
    t.load_array(np.zeros((3, h, w), np.uint8))
    padded = np.zeros((1, 64, 64), np.uint8)
    padded[0, :h, :w] = result
    t.put_batches(make_blocks_vectorized(padded, 32)[:, 0])
    assert np.array_equal(t.result, result)
    return t


def test_tiler_stats_against_an_array_and_against_polygons():
    result = _blobs(50, 60, 5, 0.05)
    rng = np.random.default_rng(3)
    rings = []
    for k in range(12):
        y, x, r = rng.uniform(5, 45), rng.uniform(5, 55), rng.uniform(1.5, 6)
        rings.append((1 + k % 2, [(x - r, y - r), (x + r, y - r), (x + r, y + r), (x - r, y + r)]))
    polys = PolygonSet.from_polygons(rings)
    burnt = rasterize_host(polys, 50, 60, all_touched=True)
    plain = _tiler_with(result).stats(classes=K, patches=True, outlines=True)
    from_array = _tiler_with(result).stats(classes=K, patches=True, outlines=True, against=burnt)
    from_polys = _tiler_with(result).stats(classes=K, patches=True, outlines=True, against=polys)
    assert plain.overlaps is None and from_array == from_polys and from_array != plain
    assert from_array.overlaps == patch_overlaps(burnt, result, K) and len(from_array.overlaps) > 3
    assert from_array.overlaps == patch_overlaps(polys, result, K)
    assert from_array.patches == plain.patches and np.array_equal(from_array.counts, plain.counts)
    assert from_array.overlaps.table_b == from_array.patches
    assert np.array_equal(from_array.outlines.xy, plain.outlines.xy)
    # the other map's configuration: default is the connectivity of `patches` without a sieve
    t = _tiler_with(result)
    st = t.stats(classes=K, patches=PatchConfig(4, 3), against=burnt)
    assert st.overlaps == patch_overlaps(burnt, t.result, K, PatchConfig(4), PatchConfig(4, 3))
    assert st.overlaps.table_b == st.patches and not np.array_equal(t.result, result)
    st = _tiler_with(result).stats(classes=K, patches=PatchConfig(4, 3), against=burnt, against_patches=PatchConfig(8, 9))
    assert st.overlaps == patch_overlaps(burnt, t.result, K, PatchConfig(8, 9), PatchConfig(4, 3))
    for bad in (dict(against=burnt), dict(patches=True, against=burnt[:, :-1]), dict(patches=True, against=burnt + 3),
                dict(patches=True, against=burnt.astype(np.int32)), dict(patches=True, against_patches=PatchConfig()),
                dict(patches=True, against=burnt, against_patches=8)):
        with pytest.raises(ValueError):
            _tiler_with(result).stats(classes=K, **bad)


class _NeverRuns:
    classes = 2

    def __getattr__(self, name):
        if name == "members":
            raise AttributeError(name)
        raise AssertionError(f"the model was touched ({name}) before the arguments were checked")


def test_infer_tile_checks_against_before_anything_runs():
    raster = np.zeros((3, 40, 40), np.uint8)
    ok = np.zeros((40, 40), np.uint8)
    for bad in (dict(stats=True, against=ok),                                      # no patches
                dict(against=ok), dict(against_patches=PatchConfig()),             # no stats
                dict(stats=True, patches=True, against=ok[:, :-1]),
                dict(stats=True, patches=True, against=ok.astype(np.int64)),
                dict(stats=True, patches=True, against=ok + 2),
                dict(stats=True, patches=True, against_patches=PatchConfig()),
                dict(stats=True, patches=True, against=ok, against_patches=True)):
        with pytest.raises(ValueError):
            infer_tile(_NeverRuns(), raster, device="cpu", **bad)
    for bad in (dict(against={0: ok}), dict(stats=True, against={0: ok}), dict(stats=True, patches=True,
                                                                               against_patches=PatchConfig())):
        with pytest.raises(ValueError):
            next(infer_rasters(_NeverRuns(), [raster], device="cpu", **bad))
