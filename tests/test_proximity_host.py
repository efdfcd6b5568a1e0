"""``deployment/proximity.py`` on the CPU.  The yardstick is a brute force written here: all pairs of a query pixel and a source
pixel in integers, O(Nq * Ns), the contract's definition read literally.  Known answers by hand, then ``patch_proximity_host``
against the brute force on the two-year 97 x 131 maps of tests/test_analysis_host.py (both directions and the gaps, with and
without a sieve and a limit), the link to ``PatchOverlaps`` (``d2 == 0`` exactly where a patch has a partner), scipy's
Euclidean distance transform as a second implementation of the distance column, the rules of the two new options from ONE
table of bad requests, and the result classes.  Integers only: every comparison is exact."""
import numpy as np
import pytest

import test_analysis_host as th
from deadtrees_amd.deployment.analysis import MapAnalysis, run_host
from deadtrees_amd.deployment.overlaps import NEW, PatchOverlaps, overlap_pairs_host
from deadtrees_amd.deployment.patches import PatchConfig, PatchTable, labelled_patches_host
from deadtrees_amd.deployment.proximity import (PatchDistances, PatchGaps, ProximityConfig, patch_distances, patch_gaps,
                                                  patch_proximity_host)
from deadtrees_amd.deployment.stats import RasterStats
from deadtrees_amd.deployment.tiler import Tiler, infer_rasters, infer_tile

K = th.K


def brute(labels_src, labels_qry, roots, exclude_own=False, limit2=None):
    """the contract's definition: per root the minimum of (d2, source root) over ALL admissible pairs"""
    sy, sx = np.nonzero(labels_src > 0)
    sl = labels_src[sy, sx].astype(np.int64)
    d2_out, near_out = [], []
    for root in np.asarray(roots).tolist():
        qy, qx = np.nonzero(labels_qry == root + 1)
        d2 = (qy[:, None] - sy[None, :]).astype(np.int64) ** 2 + (qx[:, None] - sx[None, :]).astype(np.int64) ** 2
        ok = np.ones(d2.shape, bool)
        if exclude_own:
            ok &= (sl != root + 1)[None, :]
        if limit2 is not None:
            ok &= d2 <= limit2
        key = ((d2 << 32) | (sl[None, :] - 1))[ok]               # (d2, root) in lexicographic order: d2 < 2^30, root < 2^31
        d2_out.append(int(key.min()) >> 32 if key.size else -1)
        near_out.append(int(key.min()) & 0xffffffff if key.size else -1)
    return np.array(d2_out, np.int64), np.array(near_out, np.int64)


def planes(*maps, connectivity=8):
    """uint8 class maps given as nested lists -> their int32 label planes and tables"""
    out = [labelled_patches_host(np.array(m, np.uint8), K, PatchConfig(connectivity))[1:] for m in maps]
    return out[0] if len(out) == 1 else out


def both(ls, lq, roots, exclude_own=False, limit2=None):
    got = patch_proximity_host(ls, lq, roots, exclude_own, limit2)
    want = brute(ls, lq, roots, exclude_own, limit2)
    assert got[0].dtype == got[1].dtype == np.int64
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (got, want)
    return got[0].tolist(), got[1].tolist()


# ---------------------------------------------------------------------------------------------- known answers
def test_known_answers_between_two_maps():
    one, none = planes([[1]], [[0]])
    assert both(one[0], one[0], one[1].root) == ([0], [0])                      # 1 x 1: the pixel itself
    assert both(none[0], one[0], one[1].root) == ([-1], [-1])                   # empty source
    assert both(one[0], none[0], none[1].root) == ([], [])                      # no query patch
    (la, _), (lb, tb) = planes([[1, 0, 0, 0]], [[0, 0, 0, 1]])                  # two pixels in a row
    assert both(la, lb, tb.root) == ([9], [0])
    assert both(la, lb, tb.root, limit2=9) == ([9], [0])                        # a pair at exactly the limit counts
    assert both(la, lb, tb.root, limit2=8) == ([-1], [-1])
    (la, _), (lb, tb) = planes([[1, 1, 0], [0, 0, 0]], [[0, 1, 0], [0, 1, 1]])  # overlap gives 0
    assert both(la, lb, tb.root) == ([0], [0])
    # two source patches at equal distance: the smaller root, whichever side it lies on
    (la, ta), (lb, tb) = planes([[0, 0, 0, 0, 2], [0, 0, 0, 0, 0], [1, 0, 0, 0, 0]], [[0, 0, 0, 0, 0], [0, 0, 1, 0, 0], [0] * 5])
    assert ta.root.tolist() == [4, 10] and both(la, lb, tb.root) == ([5], [4])
    (la, ta), (lb, tb) = planes([[1, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 2]], [[0, 0, 0, 0, 0], [0, 0, 1, 0, 0], [0] * 5])
    assert ta.root.tolist() == [0, 14] and both(la, lb, tb.root) == ([5], [0])
    # the up / down tie within one column: the pixel above has the smaller root; turned over, the pixel below has it
    (la, ta), (lb, tb) = planes([[0, 1], [0, 0], [0, 0], [0, 0], [0, 2]], [[0, 0], [0, 0], [1, 0], [0, 0], [0, 0]])
    assert both(la, lb, tb.root) == ([5], [1])
    assert both(la[::-1].copy(), lb[::-1].copy(), tb.root) == ([5], [1])        # labels kept, rows turned over
    assert both(np.where(la == 2, 10, np.where(la == 10, 2, 0)).astype(np.int32), lb, tb.root) == ([5], [1])


def test_known_answers_within_one_map():
    # a ring with another patch inside its hole: the ring's own pixels do not count, the inner patch is one pixel away
    ring = [[1, 1, 1, 1, 1], [1, 0, 0, 0, 1], [1, 0, 2, 0, 1], [1, 0, 0, 0, 1], [1, 1, 1, 1, 1]]
    labels, table = planes(ring)
    assert table.root.tolist() == [0, 12] and both(labels, labels, table.root, True) == ([4, 4], [12, 0])
    assert both(labels, labels, table.root, True, limit2=3) == ([-1, -1], [-1, -1])
    alone, t1 = planes([[0, 1, 1], [0, 1, 0]])
    assert both(alone, alone, t1.root, True) == ([-1], [-1])                    # no other patch
    touching, t2 = planes([[1, 2, 0], [1, 2, 0]])                               # touching classes
    assert both(touching, touching, t2.root, True) == ([1, 1], [1, 0])
    diagonal, t4 = planes([[1, 0], [0, 1]], connectivity=4)                     # connectivity 4: two patches
    assert t4.n == 2 and both(diagonal, diagonal, t4.root, True) == ([2, 2], [3, 0])
    assert planes([[1, 0], [0, 1]])[1].n == 1                                   # connectivity 8: one
    # three patches in a column: for the top one the nearest OTHER label lies behind a stretch of its own
    column, t3 = planes([[1], [1], [0], [2], [1]])
    assert t3.n == 3 and both(column, column, t3.root, True) == ([4, 1, 1], [3, 4, 3])


def test_bad_planes_are_refused():
    ok = np.zeros((3, 4), np.int32)
    for src, qry, limit2, fragment in ((ok.astype(np.int64), ok, None, "int32"), (ok, ok[:, :3], None, "one grid"),
                                       (ok[:0], ok[:0], None, "sides"), (ok, ok, -1, "limit2"), (ok, ok, 2.5, "limit2")):
        with pytest.raises(ValueError, match=fragment):
            patch_proximity_host(src, qry, [], False, limit2)


# ---------------------------------------------------------------------------------------------- against the brute force
@pytest.fixture(scope="module")
def years():
    """the label planes and tables of the two years, unsieved / sieved: ``{sieved: ((la, ta), (lb, tb))}``"""
    a, b, _ = th.two_years()
    return {False: (labelled_patches_host(a, K, PatchConfig(8))[1:], labelled_patches_host(b, K, PatchConfig(8))[1:]),
            True: (labelled_patches_host(a, K, PatchConfig(8, 3))[1:], labelled_patches_host(b, K, PatchConfig(4, 6))[1:])}


@pytest.mark.parametrize("limit2", [None, 20])
@pytest.mark.parametrize("sieved", [False, True])
def test_two_years_equal_the_brute_force(years, sieved, limit2):
    (la, ta), (lb, tb) = years[sieved]
    d2_b, near_b = both(la, lb, tb.root, limit2=limit2)
    d2_a, _ = both(lb, la, ta.root, limit2=limit2)
    gap_b, _ = both(lb, lb, tb.root, True, limit2)
    # worth comparing: overlaps, patches apart, and under the limit patches without a neighbour (counted by the brute force)
    assert 0 in d2_b and max(d2_b) > 0 and 0 in d2_a and max(d2_a) > 0 and 1 in gap_b and max(gap_b) > 2
    without = {(False, None): (0, 0, 0), (False, 20): (3, 0, 0), (True, None): (0, 0, 0), (True, 20): (0, 29, 33)}
    assert (d2_b.count(-1), d2_a.count(-1), gap_b.count(-1)) == without[sieved, limit2]
    if limit2 is None:
        # d2 == 0 exactly for the patches with a partner
        pairs = PatchOverlaps(ta, tb, *overlap_pairs_host(la, lb))
        assert np.array_equal(np.array(d2_b) == 0, pairs.partners_b() > 0)
        assert np.array_equal(np.array(d2_a) == 0, pairs.partners_a() > 0)
        # the distance column from scipy's Euclidean distance transform
        from scipy.ndimage import distance_transform_edt
        edt2 = np.rint(distance_transform_edt(la == 0) ** 2).astype(np.int64)
        want = np.full(tb.n, np.iinfo(np.int64).max)
        np.minimum.at(want, np.searchsorted(tb.root, lb[lb > 0] - 1), edt2[lb > 0])
        assert np.array_equal(want, d2_b)
        assert set(near_b) <= set(ta.root.tolist())


def test_maps_in_objects_out_and_the_host_runner(years):
    a, b, zones = th.two_years()
    (la, ta), (lb, tb) = years[True]
    limit = ProximityConfig(4.5)
    assert limit.limit2 == 20 and ProximityConfig().limit2 is None and ProximityConfig(3).limit2 == 9
    assert ProximityConfig(0).limit2 == 0 and ProximityConfig(np.sqrt(2)).limit2 == 2
    for bad in (-1, "far", True, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="max_distance"):
            ProximityConfig(bad)
    with pytest.raises(Exception):
        limit.max_distance = 2                                   # frozen
    apart = patch_distances(a, b, K, PatchConfig(8, 3), PatchConfig(4, 6), limit)
    assert apart.table_a == ta and apart.table_b == tb
    d2, near = brute(la, lb, tb.root, limit2=20)
    assert np.array_equal(apart.b_d2, d2)
    assert np.array_equal(apart.b_nearest, np.where(near < 0, -1, np.searchsorted(ta.root, near)))
    d2, near = brute(lb, la, ta.root, limit2=20)
    assert np.array_equal(apart.a_d2, d2)
    assert np.array_equal(apart.a_nearest, np.where(near < 0, -1, np.searchsorted(tb.root, near)))
    gaps = patch_gaps(b, K, PatchConfig(4, 6), limit)
    d2, near = brute(lb, lb, tb.root, True, 20)
    assert gaps.table == tb and np.array_equal(gaps.d2, d2)
    assert np.array_equal(gaps.nearest, np.where(near < 0, -1, np.searchsorted(tb.root, near)))
    assert patch_gaps(b, K, PatchConfig(4, 6)) != gaps and patch_distances(a, b, K, PatchConfig(8, 3), PatchConfig(4, 6)) != apart
    with pytest.raises(ValueError, match="ProximityConfig"):
        patch_gaps(b, K, proximity=4.5)
    with pytest.raises(ValueError, match="out of range"):
        patch_distances(a, b + K, K)
    # the host runner strings the same together; without the options everything is what it was
    options = dict(zones=zones, patches=PatchConfig(4, 6), outlines=True, against=a, against_patches=PatchConfig(8, 3))
    plain_map, plain = run_host(MapAnalysis.of("caller", b.shape, K, **options), b)
    full_map, full = run_host(MapAnalysis.of("caller", b.shape, K, distances=limit, gaps=limit, **options), b)
    assert full.overlaps.distances == apart and full.gaps == gaps and np.array_equal(full_map, plain_map)
    assert plain.gaps is None and plain.overlaps.distances is None and plain != full and plain.overlaps != full.overlaps
    assert full.patches == plain.patches and np.array_equal(full.counts, plain.counts)
    assert np.array_equal(full.outlines.xy, plain.outlines.xy)
    assert all(np.array_equal(getattr(full.overlaps, c), getattr(plain.overlaps, c)) for c in "abn")
    only_gaps = run_host(MapAnalysis.of("caller", b.shape, K, patches=PatchConfig(4, 6), gaps=True), b)[1]
    assert only_gaps.gaps == patch_gaps(b, K, PatchConfig(4, 6)) and only_gaps.overlaps is None
    unlimited = run_host(MapAnalysis.of("caller", b.shape, K, distances=True, **options), b)[1]
    assert unlimited.gaps is None and unlimited.overlaps.distances == patch_distances(a, b, K, PatchConfig(8, 3), PatchConfig(4, 6))
    # repr / == / + without the options are what they were
    assert "gaps" not in repr(plain) and "distances" not in repr(plain) and "distances" not in repr(plain.overlaps)
    assert "gaps=PatchGaps(n=132" in repr(full) and "distances=PatchDistances(n_a=" in repr(full.overlaps)
    assert repr(plain.overlaps) == (f"PatchOverlaps(pairs={len(plain.overlaps)}, n_a={ta.n}, n_b={tb.n}, "
                                    f"shared pixels={int(plain.overlaps.n.sum())})")
    again = RasterStats(plain.counts, patches=plain.patches, outlines=plain.outlines, overlaps=plain.overlaps)
    assert again == plain and repr(again) == repr(plain)
    total = full + full
    assert total.gaps is None and total.overlaps is None and total == plain + plain
    with pytest.raises(ValueError, match="gaps"):
        RasterStats(plain.counts, patches=plain.patches, gaps=patch_gaps(a, K))
    with pytest.raises(ValueError, match="distances"):
        PatchOverlaps(ta, tb, *overlap_pairs_host(la, lb), distances=patch_distances(b, a, K))


# ---------------------------------------------------------------------------------------------- the options' rules
OK = th.OK
BAD = [
    ("distances without stats", dict(distances=True), "stats=True"),
    ("gaps without stats", dict(gaps=True), "stats=True"),
    ("a gaps configuration without stats", dict(gaps=ProximityConfig(3)), "stats=True"),
    ("gaps without patches", dict(stats=True, gaps=True), "gaps need patches"),
    ("distances without against", dict(stats=True, patches=True, distances=True), "distances need against"),
    ("distances without against or patches", dict(stats=True, distances=ProximityConfig(2)), "distances need against"),
    ("distances without patches", dict(stats=True, against=OK, distances=True), "against needs patches"),
    ("distances that are a number", dict(stats=True, patches=True, against=OK, distances=12.5), "distances must be"),
    ("gaps that are a PatchConfig", dict(stats=True, patches=True, gaps=PatchConfig()), "gaps must be"),
]


@pytest.mark.parametrize("what,options,fragment", BAD, ids=[what.replace(" ", "-") for what, _, _ in BAD])
def test_every_entry_point_refuses_a_bad_request(what, options, fragment):
    raster = np.zeros((3, th.H, th.W), np.uint8)
    for who in ("caller", "Tiler.stats"):
        with pytest.raises(ValueError, match=f"^{who}: .*{fragment}"):
            MapAnalysis.of(who, (th.H, th.W), K, **{"stats": False, **options})
    with pytest.raises(ValueError, match=f"^infer_tile: .*{fragment}"):
        infer_tile(th._NeverRuns(), raster, device="cpu", **options)
    per_key = {k: ({0: v} if k == "against" else v) for k, v in options.items()}
    queue = infer_rasters(th._NeverRuns(), [raster], device="cpu", **per_key)
    with pytest.raises(ValueError, match=f"^infer_rasters: .*{fragment}"):
        next(queue)
    if options.get("stats"):
        t = Tiler(tile_shape=(64, 64), subtile_shape=(32, 32))
        t.load_array(raster[:1])
        with pytest.raises(ValueError, match=f"^Tiler.stats: .*{fragment}"):
            t.stats(classes=K, **{k: v for k, v in options.items() if k != "stats"})


def test_a_valid_request_reads_back_by_name():
    plain = MapAnalysis.of("caller", (th.H, th.W), K, patches=True, against=OK)
    assert plain.distances is None and plain.gaps is None
    full = MapAnalysis.of("caller", (th.H, th.W), K, patches=True, against=OK, distances=True, gaps=ProximityConfig(7))
    assert full.distances == ProximityConfig() and full.gaps == ProximityConfig(7) and full.gaps.limit2 == 49
    assert MapAnalysis.of("caller", (th.H, th.W), K, patches=True, gaps=False, distances=None).gaps is None
    # a raster of infer_rasters without a map to compare with has no distances, but keeps its gaps
    rules = MapAnalysis.rules("caller", K, True, None, None, True, None, {}, None, True, True)
    bound = rules.bind("caller", (th.H, th.W), None, None)
    assert bound.distances is None and bound.gaps == ProximityConfig()
    assert rules.bind("caller", (th.H, th.W), None, OK).distances == ProximityConfig()
    t = Tiler(tile_shape=(64, 64), subtile_shape=(32, 32))
    t.load_array(np.zeros((1, th.H, th.W), np.uint8))
    t.result[2:4, 2:5], t.result[10, 10] = 1, 2
    before = OK.copy()
    before[20, 30] = 1
    stats = t.stats(classes=K, patches=True, against=before, distances=True, gaps=ProximityConfig(10))
    assert stats.gaps == patch_gaps(t.result, K, proximity=ProximityConfig(10)) == PatchGaps(stats.patches, [85, 85], [1, 0])
    assert stats.overlaps.distances == patch_distances(before, t.result, K)
    assert stats.overlaps.distances.b_d2.tolist() == [26 * 26 + 17 * 17, 500] and len(stats.overlaps) == 0


# ---------------------------------------------------------------------------------------------- the result classes
def test_histograms_and_metres_on_a_hand_case():
    def table(areas):
        n = len(areas)
        return PatchTable(np.arange(n) * 7, np.ones(n, np.uint8), np.array(areas), np.zeros((n, 4), np.int32),
                          np.zeros(n, np.int64), np.zeros(n, np.int64), shape=(20, 20))
    ta, tb = table([5, 6]), table([1, 2, 3, 4])
    apart = PatchDistances(ta, tb, [0, 25], [1, 3], [0, 9, -1, 16], [0, 0, -1, 1])
    assert np.array_equal(apart.a_distance(), [0.0, 5.0])
    assert np.array_equal(apart.b_distance(), [0.0, 3.0, np.nan, 4.0], equal_nan=True)
    assert np.array_equal(apart.b_distance_m(), np.array([0.0, 3.0, np.nan, 4.0]) * 0.2, equal_nan=True)
    assert np.array_equal(apart.a_distance_m(0.5), [0.0, 2.5])
    # bands: < 1, 1 <= . < 4, >= 4 pixels; a patch without a distance is in no band
    assert apart.histogram([1, 4]).tolist() == [1, 1, 1] and apart.histogram([1, 4], side="a").tolist() == [1, 0, 1]
    assert apart.histogram([1, 4], weights="area").tolist() == [1, 2, 4]
    assert apart.histogram([1, 4], side="a", weights="area").tolist() == [5, 0, 6]
    new = np.array([NEW, 1, NEW, NEW]) == NEW
    assert apart.histogram([1, 4], only=new).tolist() == [1, 0, 1] and apart.histogram([3.5], only=new).tolist() == [1, 1]
    assert apart.histogram([3], weights="area").tolist() == [1, 6]              # an edge belongs to the band above it
    for bad in (dict(edges=[]), dict(edges=[2, 1]), dict(edges=[1], side="c"), dict(edges=[1], weights="pixels"),
                dict(edges=[1], only=[1, 0, 1, 0]), dict(edges=[1], only=np.ones(3, bool))):
        with pytest.raises(ValueError, match="histogram"):
            apart.histogram(**bad)
    assert apart == PatchDistances(ta, tb, [0, 25], [1, 3], [0, 9, -1, 16], [0, 0, -1, 1])
    assert apart != PatchDistances(ta, tb, [0, 25], [1, 3], [0, 9, -1, 16], [0, 0, -1, 0]) and apart != "apart"
    assert repr(apart) == ("PatchDistances(n_a=2, n_b=4, a: 1 touching, 1 apart, 0 without, farthest 5.0 px, "
                           "b: 1 touching, 2 apart, 1 without, farthest 4.0 px)")
    for bad in (([0], [1], [0, 9, -1, 16], [0, 0, -1, 1]), ([0, 25], [1, 4], [0, 9, -1, 16], [0, 0, -1, 1]),
                ([0, 25], [1, 3], [0, 9, -1, 16], [0, 0, 1, 1]), ([0, -1], [1, 3], [0, 9, -1, 16], [0, 0, -1, 1])):
        with pytest.raises(ValueError, match="PatchDistances"):
            PatchDistances(ta, tb, *bad)
    with pytest.raises(ValueError, match="missing"):
        PatchDistances.from_roots(ta, tb, ([0, 25], [7, 8]), ([0, 9, -1, 16], [0, 0, -1, 7]))
    assert PatchDistances.from_roots(ta, tb, ([0, 25], [7, 21]), ([0, 9, -1, 16], [0, 0, -1, 7])) == apart
    gaps = PatchGaps(tb, [1, 1, -1, 8], [1, 0, -1, 2])
    assert np.array_equal(gaps.distance(), [1.0, 1.0, np.nan, np.sqrt(8.0)], equal_nan=True)
    assert np.array_equal(gaps.distance_m(1.0), gaps.distance(), equal_nan=True)
    assert gaps.histogram([2]).tolist() == [2, 1] and gaps.histogram([2], weights="area", only=new).tolist() == [1, 4]
    assert gaps == PatchGaps.from_roots(tb, ([1, 1, -1, 8], [7, 0, -1, 14])) and gaps != PatchGaps(tb, [1, 1, -1, 8], [1, 0, -1, 1])
    assert repr(gaps) == "PatchGaps(n=4, 2 touching, 1 apart, 1 without, farthest 2.8 px)"
    for bad in (([0, 1, -1, 8], [1, 0, -1, 2]), ([1, 1, -1, 8], [0, 0, -1, 2])):
        with pytest.raises(ValueError, match="own neighbour"):
            PatchGaps(tb, *bad)
