"""The crown split on the host (``deployment/crowns.py``): the contract's known answers number for number, ``depth2_host``
against a scalar brute force, ``split_patches_host`` against a scalar queue-based restatement of steps 3 to 6, the contract's
properties on seeded random maps, the errors of ``CrownConfig`` and ``MapAnalysis.rules``, ``run_host`` against the by-hand
pipeline, and ``RasterStats`` with and without ``crowns``.  Integers only: every comparison is exact."""
from fractions import Fraction

import numpy as np
import pytest

from deadtrees_amd.data.polygons import rasterize
from deadtrees_amd.deployment.analysis import MapAnalysis, run_host
from deadtrees_amd.deployment.crowns import (CrownConfig, CrownSplit, check_crowns, crown_depths_host, depth2_host,
                                             split_patches, split_patches_host)
from deadtrees_amd.deployment.outlines import outlines_from_labels
from deadtrees_amd.deployment.overlaps import PatchOverlaps, overlap_pairs_host
from deadtrees_amd.deployment.patches import (PatchConfig, label_patches_host, labelled_patches_host, measure_patches_host,
                                              sieve_host)
from deadtrees_amd.deployment.proximity import gaps_of
from deadtrees_amd.deployment.stats import RasterStats, zonal_counts_host


# ---------------------------------------------------------------------------------------------- maps
def two_discs(h=24, w=36, centres=((12, 12), (12, 22)), r2=36, cls=1):
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), np.uint8)
    for cy, cx in centres:
        m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r2] = cls
    return m


def lobe_bar(h=16, w=48, lobe=33):
    m = np.zeros((h, w), np.uint8)
    m[2:13, 2:13] = 1
    m[7, 13:13 + lobe] = 1
    return m


def random_map(h, w, K, seed, cover=0.5, grow=2):
    """blobs: seeds dilated ``grow`` times, classes drawn per seed, so that patches have necks and touch"""
    from scipy import ndimage
    rng = np.random.default_rng(seed)
    m = np.zeros((h, w), np.uint8)
    for c in range(1, K):
        seeds = rng.random((h, w)) < cover / (K - 1) / (2 * grow + 1) ** 2
        blob = ndimage.binary_dilation(seeds, iterations=grow) if grow else seeds
        m[blob & (rng.random((h, w)) < 0.97)] = c
    return m


def split(m, K, connectivity, config):
    lp = label_patches_host(m, K, connectivity)
    return (lp,) + split_patches_host(m, lp, K, connectivity, config)


# ---------------------------------------------------------------------------------------------- known answers
def test_two_discs_number_for_number():
    m = two_discs()
    d2 = depth2_host(m, 2)
    assert int(m.sum()) == 217 and int(d2.max()) == 37 and int(d2[:, 17].max()) <= 16
    for E, want in ((1, 1), (4, 1), (9, 1), (16, 1), (25, 2), (36, 2), (49, 1)):
        lp, crowns, depth2, converged = split(m, 2, 8, CrownConfig(E, 12))
        table = measure_patches_host(crowns, m)
        assert table.n == want and converged, E
        assert np.array_equal(depth2, d2)
        if want == 1:
            assert np.array_equal(crowns, lp)
        if E == 25:
            assert table.root.tolist() == [228, 238] and table.area.tolist() == [112, 105]


def test_lobe_bar_number_for_number():
    m = lobe_bar()
    lp, crowns, _, converged = split(m, 2, 8, CrownConfig(9, 2))
    table = measure_patches_host(crowns, m)
    assert table.root.tolist() == [98, 349] and table.area.tolist() == [121, 33] and not converged
    lp, crowns, _, converged = split(m, 2, 8, CrownConfig(9, 40))
    table = measure_patches_host(crowns, m)
    assert table.root.tolist() == [98] and table.area.tolist() == [154] and converged and np.array_equal(crowns, lp)


# ---------------------------------------------------------------------------------------------- depth
def depth2_brute(m, cap2):
    h, w = m.shape
    out = np.zeros((h, w), np.int32)
    for y in range(h):
        for x in range(w):
            if m[y, x] == 0:
                continue
            best = cap2
            for qy in range(h):
                for qx in range(w):
                    if m[qy, qx] != m[y, x]:
                        best = min(best, (y - qy) ** 2 + (x - qx) ** 2)
            out[y, x] = best
    return out


@pytest.mark.parametrize("case", ["random 0", "random 1", "random 2", "uniform", "edge", "capped"])
def test_depth2_against_brute_force(case):
    cap2 = 65535
    if case.startswith("random"):
        seed = int(case[-1])
        m = random_map((9, 24, 17)[seed], (31, 13, 20)[seed], 3, seed, cover=(0.4, 0.9, 1.5)[seed])
    elif case == "uniform":
        m = np.full((7, 11), 2, np.uint8)
    elif case == "edge":
        m = np.zeros((12, 15), np.uint8)
        m[0:7, 0:9] = 1                                           # cut by two raster edges: the outside does not count
        m[5:12, 11:15] = 2
    else:
        m, cap2 = two_discs(), 10
    got = depth2_host(m, 3, cap2)
    assert got.dtype == np.int32 and np.array_equal(got, depth2_brute(m, cap2))
    if case == "uniform":
        assert (got == cap2).all()
    if case == "edge":
        assert got[0, 0] == 49 and got[3, 0] == 16
    if case == "capped":
        assert int(got.max()) == 10 and int(depth2_host(m, 3).max()) == 37


# ---------------------------------------------------------------------------------------------- steps 3 to 6, scalar
def split_scalar(m, core_labels, connectivity, max_rounds):
    """steps 3 to 6 pixel by pixel: growth with a frontier queue per round, the remainder by flood fill, canonical labels"""
    h, w = m.shape
    near = [(-1, 0), (0, -1), (0, 1), (1, 0)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])

    def around(y, x):
        for dy, dx in near:
            if 0 <= y + dy < h and 0 <= x + dx < w and m[y + dy, x + dx] == m[y, x]:
                yield y + dy, x + dx

    S = {(y, x): int(core_labels[y, x]) for y in range(h) for x in range(w) if core_labels[y, x]}
    frontier = list(S)
    for _ in range(max_rounds):
        offers = {}
        for y, x in frontier:                                     # only last round's pixels can offer something new
            for q in around(y, x):
                if q not in S:
                    offers.setdefault(q, None)
        for q in offers:
            offers[q] = min(S[n] for n in around(*q) if n in S)
        if not offers:
            break
        S.update(offers)
        frontier = list(offers)
    converged = not any(q not in S for p in S for q in around(*p))
    seg, next_id = dict(S), -1
    for y in range(h):
        for x in range(w):
            if m[y, x] and (y, x) not in seg:
                stack, seg[(y, x)] = [(y, x)], next_id
                while stack:
                    for q in around(*stack.pop()):
                        if q not in seg:
                            seg[q] = next_id
                            stack.append(q)
                next_id -= 1
    first = {}
    for (y, x), s in sorted(seg.items()):
        first.setdefault(s, y * w + x)
    out = np.zeros((h, w), np.int32)
    for (y, x), s in seg.items():
        out[y, x] = first[s] + 1
    return out, converged


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("E, max_rounds", [(4, 256), (9, 1), (9, 3), (2, 0), (16, 256)])
def test_split_against_scalar_restatement(connectivity, E, max_rounds):
    for seed in range(3):
        m = random_map(23, 30, 3, 40 + seed, cover=1.2, grow=2 + seed % 2)
        lp, crowns, depth2, converged = split(m, 3, connectivity, CrownConfig(E, max_rounds))
        cores = label_patches_host(np.where(depth2 >= E, m, 0).astype(np.uint8), 3, connectivity)
        want, want_converged = split_scalar(m, cores, connectivity, max_rounds)
        assert np.array_equal(crowns, want) and converged == want_converged


# ---------------------------------------------------------------------------------------------- properties
CONFIGS = [(4, 256), (9, 256), (9, 2), (25, 1)]


@pytest.mark.parametrize("seed", range(30))
def test_properties_on_random_maps(seed):
    K, connectivity = 2 + seed % 2, (4, 8)[(seed // 2) % 2]
    m = random_map(20 + seed % 7, 26 + seed % 5, K, seed, cover=0.8 + 0.1 * (seed % 4), grow=1 + seed % 3)
    lp = label_patches_host(m, K, connectivity)
    top = int(depth2_host(m, K).max())
    for E, rounds in ((1, 256), (top + 1, 256)):                  # no neck is cut, and no patch has a core
        assert np.array_equal(split_patches_host(m, lp, K, connectivity, CrownConfig(E, rounds))[0], lp)
    for E, rounds in CONFIGS:
        crowns, depth2, converged = split_patches_host(m, lp, K, connectivity, CrownConfig(E, rounds))
        table = measure_patches_host(crowns, m)                   # the label contract: accepted as it is
        assert crowns.dtype == np.int32 and ((crowns != 0) == (m != 0)).all()
        flat, lpf, mf = crowns.ravel(), lp.ravel(), m.ravel()
        for root in table.root:
            inside = flat == root + 1
            assert len(np.unique(lpf[inside])) == 1 and len(np.unique(mf[inside])) == 1      # one patch, one class
            alone = label_patches_host(inside.reshape(m.shape).astype(np.uint8), 2, connectivity)
            assert len(np.unique(alone[alone != 0])) == 1                                    # connected
        a, b, n = overlap_pairs_host(lp, crowns)                  # ascending in (patch, crown): one row per crown
        order = np.argsort(b, kind="stable")
        assert np.array_equal(b[order], table.root) and np.array_equal(n[order], table.area)
        assert np.array_equal(a[order], lpf[table.root] - 1)
        rings = outlines_from_labels(crowns, m, connectivity)
        assert len(rings) == table.n and np.array_equal(rasterize(rings, m.shape, all_touched=False), m)
        if converged and rounds == 256:                          # a patch without a core keeps its label
            cores = depth2 >= E
            for root in np.unique(lp[lp != 0]) - 1:
                if not cores[lp == root + 1].any():
                    assert (crowns[lp == root + 1] == root + 1).all()


def test_parent_root_and_crown_split():
    m = np.zeros((30, 60), np.uint8)
    m[3:27, 2:38] = two_discs()
    m[10:20, 45:55] = 2
    config = CrownConfig(25, 12)
    classes, crowns, table, got = labelled_patches_host(m, 3, PatchConfig(8), crowns=config)
    lp = label_patches_host(m, 3, 8)
    assert classes is not None and table.n == 3 and got.n == 3 and got.n_patches == 2 and got.converged
    assert np.array_equal(got.parent_root, lp.ravel()[table.root] - 1) and got.parent_root.dtype == np.int64
    assert got.parent_root[0] == got.parent_root[1] == table.root[0] != got.parent_root[2]
    depth2 = depth2_host(m, 3)
    assert got.depth2.dtype == np.int32 and got.depth2.tolist() == [int(depth2[crowns == r + 1].max()) for r in table.root]
    assert np.array_equal(got.radius(), np.sqrt(got.depth2)) and got.depth2[2] == 25
    assert np.array_equal(crown_depths_host(crowns, depth2)[table.root], got.depth2)
    assert repr(got) == "CrownSplit(n=3, n_patches=2, converged=True, min_core2=25)"
    assert got == CrownSplit(table, got.parent_root, got.depth2, True, config)
    assert got != CrownSplit(table, got.parent_root, got.depth2, False, config)
    assert got != CrownSplit(table, got.parent_root, got.depth2, True, CrownConfig(25, 13))
    with pytest.raises(ValueError, match="CrownSplit: depth2 must hold one entry per crown"):
        CrownSplit(table, got.parent_root, got.depth2[:2], True, config)
    with pytest.raises(ValueError, match="CrownSplit: table must be a PatchTable"):
        CrownSplit(None, [], [], True, config)
    # the stand-alone entry; a pixel of its own has no core and stays a crown
    alone, split_alone = split_patches(m, 3, config)
    assert np.array_equal(alone, crowns) and split_alone == got
    m[0, 59] = 1
    assert split_patches(m, 3, config)[1].n == 4
    with pytest.raises(ValueError, match="split_patches: config must be a CrownConfig"):
        split_patches(m, 3, 25)


# ---------------------------------------------------------------------------------------------- errors
def test_crown_config():
    c = CrownConfig(9)
    assert (c.min_core2, c.max_rounds, c.depth_cap2) == (9, 256, 65535)
    assert repr(c) == "CrownConfig(min_core2=9, max_rounds=256, depth_cap2=65535)"
    assert c == CrownConfig(9, 256, 65535) and c != CrownConfig(9, 255) and c != CrownConfig(8) and c != CrownConfig(9, 256, 9)
    assert c != 9
    with pytest.raises(TypeError):
        hash(c)
    assert CrownConfig.from_radius(2) == CrownConfig(4) and CrownConfig.from_radius(2.5) == CrownConfig(7)
    assert CrownConfig.from_radius(Fraction(7, 2)).min_core2 == 13 and CrownConfig.from_radius(0.1).min_core2 == 1
    assert CrownConfig.from_radius(3.0000000000000004).min_core2 == 10      # exact: the float is above 3
    assert CrownConfig(2 ** 30, 0, 2 ** 30).max_rounds == 0
    for bad in (0, -1, True, 2.0, "9", None, 65536):
        with pytest.raises(ValueError, match="CrownConfig: min_core2"):
            CrownConfig(bad)
    for bad in (-1, True, 1.5, None):
        with pytest.raises(ValueError, match="CrownConfig: max_rounds"):
            CrownConfig(9, bad)
    for bad in (0, 2 ** 30 + 1, True, 4.0):
        with pytest.raises(ValueError, match="CrownConfig: depth_cap2"):
            CrownConfig(1, 256, bad)
    for bad in (0, -2, True, "2", float("inf"), float("nan")):
        with pytest.raises(ValueError, match="CrownConfig.from_radius"):
            CrownConfig.from_radius(bad)
    assert check_crowns(None) is None and check_crowns(False) is None and check_crowns(c) is c
    assert check_crowns(True) == CrownConfig(4)
    with pytest.raises(ValueError, match="crowns must be True, False, None or a CrownConfig, got 9"):
        check_crowns(9)


def test_host_argument_errors():
    m = two_discs()
    lp = label_patches_host(m, 2, 8)
    with pytest.raises(ValueError, match="split_patches: config must be a CrownConfig"):
        split_patches_host(m, lp, 2, 8, 9)
    with pytest.raises(ValueError, match="split_patches: connectivity must be 4 or 8"):
        split_patches_host(m, lp, 2, 6, CrownConfig(9))
    with pytest.raises(ValueError, match="split_patches: labels must be int32"):
        split_patches_host(m, lp.astype(np.int64), 2, 8, CrownConfig(9))
    with pytest.raises(ValueError, match="split_patches: labels and classes do not belong together"):
        split_patches_host(m, np.zeros_like(lp), 2, 8, CrownConfig(9))
    with pytest.raises(ValueError, match="split_patches: class value 2 out of range"):
        split_patches_host(m * 2, lp, 2, 8, CrownConfig(9))
    with pytest.raises(ValueError, match="depth2: K must be in 2..8"):
        depth2_host(m, 9)
    with pytest.raises(ValueError, match="depth2: cap2"):
        depth2_host(m, 2, 0)
    with pytest.raises(ValueError, match="depth2: classes must be uint8"):
        depth2_host(m.astype(np.int32), 2)


def test_rules_errors_name_the_caller():
    rules = MapAnalysis.rules
    with pytest.raises(ValueError, match="caller: crowns must be True, False, None or a CrownConfig, got 9"):
        rules("caller", 2, patches=True, crowns=9)
    with pytest.raises(ValueError, match="caller: against_crowns must be True, False, None or a CrownConfig"):
        rules("caller", 2, patches=True, against=object(), against_crowns=PatchConfig())
    with pytest.raises(ValueError, match="caller: crowns / against_crowns need stats=True"):
        rules("caller", 2, stats=False, crowns=True)
    with pytest.raises(ValueError, match="caller: crowns need patches"):
        rules("caller", 2, crowns=CrownConfig(9))
    with pytest.raises(ValueError, match="caller: against_crowns needs patches and against"):
        rules("caller", 2, patches=True, against_crowns=CrownConfig(9))
    got = rules("caller", 2, patches=True, crowns=True, against=object(), against_crowns=CrownConfig(9))
    assert got.crowns == CrownConfig(4) and got.against_crowns == CrownConfig(9)
    plain = rules("caller", 2, patches=True)
    assert plain.crowns is None and plain.against_crowns is None
    # a raster without `against` drops the option, as it drops against_patches
    bound = rules("caller", 2, patches=True, against=object(), against_crowns=True).bind("caller", (4, 4))
    assert bound.against_crowns is None and bound.against_patches is None


def test_entry_points_check_before_anything_runs():
    from deadtrees_amd.deployment.tiler import Tiler, infer_rasters, infer_tile
    raster = np.zeros((3, 8, 8), np.uint8)

    class Model:
        classes = 2

    with pytest.raises(ValueError, match="infer_tile: crowns must be"):
        infer_tile(Model(), raster, stats=True, patches=True, crowns=3)
    with pytest.raises(ValueError, match="infer_tile: crowns need patches"):
        infer_tile(Model(), raster, stats=True, crowns=True)
    with pytest.raises(ValueError, match="infer_rasters: against_crowns needs patches and against"):
        next(infer_rasters(Model(), [raster], stats=True, patches=True, against_crowns=True))
    t = Tiler(tile_shape=(8, 8), subtile_shape=(4, 4))
    t.load_array(raster)
    with pytest.raises(ValueError, match="Tiler.stats: crowns must be"):
        t.stats(classes=2, patches=True, crowns="yes")
    t.put_batches(np.ones((4, 4, 4), np.uint8))
    stats = t.stats(classes=2, patches=True, crowns=CrownConfig(4))
    assert stats.crowns.n == 1 and stats.crowns.depth2.tolist() == [65535] and stats.patches.n == 1


# ---------------------------------------------------------------------------------------------- run_host, RasterStats
def _year_maps():
    b = random_map(40, 56, 3, 7, cover=1.0, grow=3)
    a = random_map(40, 56, 3, 8, cover=1.0, grow=3)
    b[8:32, 10:46] = two_discs()                                  # one patch that E = 25 cuts in two
    b[0, 0], b[0, 2] = 1, 2                                       # speckle for the sieve
    return a, b


def test_run_host_equals_the_pipeline_by_hand():
    a, b = _year_maps()
    K, config, crowns, crowns_a = 3, PatchConfig(8, 4), CrownConfig(25), CrownConfig(4, 3)
    request = MapAnalysis.of("caller", b.shape, K, patches=config, outlines=True, against=a, gaps=True, crowns=crowns,
                             against_crowns=crowns_a)
    got_map, got = run_host(request, b)
    lp = label_patches_host(b, K, 8)
    sieved, lp = sieve_host(b, lp, 4)
    plane, depth2, converged = split_patches_host(sieved, lp, K, 8, crowns)
    table = measure_patches_host(plane, sieved)
    assert np.array_equal(got_map, sieved) and got.patches == table and table.n > measure_patches_host(lp, sieved).n
    assert got.crowns == CrownSplit(table, lp.ravel()[table.root] - 1, crown_depths_host(plane, depth2)[table.root], converged,
                                    crowns)
    assert got.crowns.n_patches == measure_patches_host(lp, sieved).n
    assert np.array_equal(got.counts, zonal_counts_host(sieved, None, K, 1))
    la = label_patches_host(a, K, 8)
    plane_a = split_patches_host(a, la, K, 8, crowns_a)[0]
    assert got.overlaps == PatchOverlaps(measure_patches_host(plane_a, a), table, *overlap_pairs_host(plane_a, plane))
    assert got.gaps == gaps_of(plane, table)
    want_rings = outlines_from_labels(plane, sieved, 8)
    assert all(np.array_equal(getattr(got.outlines, f), getattr(want_rings, f))
               for f in ("xy", "ring_offsets", "ring_polygon", "values"))
    # without the options: the request of today, object for object
    options = dict(patches=config, outlines=True, against=a, gaps=True)
    plain_map, plain = run_host(MapAnalysis.of("caller", b.shape, K, **options), b)
    off_map, off = run_host(MapAnalysis.of("caller", b.shape, K, crowns=None, against_crowns=False, **options), b)
    assert np.array_equal(plain_map, off_map) and np.array_equal(plain_map, got_map)
    assert plain == off and repr(plain) == repr(off) and plain.crowns is None and "crowns" not in repr(plain)
    assert plain.patches == measure_patches_host(lp, sieved) and plain != got and np.array_equal(plain.counts, got.counts)
    # only the other map is split
    only_a = run_host(MapAnalysis.of("caller", b.shape, K, against_crowns=crowns_a, **options), b)[1]
    assert only_a.patches == plain.patches and only_a.crowns is None and only_a.overlaps.table_a == got.overlaps.table_a


def test_raster_stats_with_and_without_crowns():
    _, b = _year_maps()
    K = 3
    _, plane, table, crowns = labelled_patches_host(b, K, PatchConfig(8), crowns=CrownConfig(25))
    counts = zonal_counts_host(b, None, K, 1)
    with_crowns = RasterStats(counts, patches=table, crowns=crowns)
    without = RasterStats(counts, patches=table)
    assert with_crowns.crowns is crowns and without.crowns is None
    assert with_crowns == RasterStats(counts, patches=table, crowns=crowns) and with_crowns != without and without != with_crowns
    assert repr(with_crowns) == repr(without)[:-1] + f", crowns={crowns!r})" and "crowns" not in repr(without)
    total = with_crowns + without
    assert total.crowns is None and total.patches is None and np.array_equal(total.counts, 2 * counts)
    assert total == without + without
    with pytest.raises(ValueError, match="RasterStats: crowns must be a CrownSplit or None, got PatchConfig"):
        RasterStats(counts, patches=table, crowns=PatchConfig())
    with pytest.raises(ValueError, match="RasterStats: crowns need the PatchTable they belong to"):
        RasterStats(counts, crowns=crowns)
    other = labelled_patches_host(b, K, PatchConfig(8))[2]
    with pytest.raises(ValueError, match="RasterStats: crowns need the PatchTable they belong to"):
        RasterStats(counts, patches=other, crowns=crowns)
