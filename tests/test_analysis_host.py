"""``deployment/analysis.py`` on the CPU: every rule of the statistics options from ONE table of bad requests, raised alike by
``MapAnalysis.of``, ``infer_tile``, ``infer_rasters`` and ``Tiler.stats``; a valid request read back by name; ``run_host``
against the direct composition of the host functions it strings together.  Integers only: every comparison is exact."""
import numpy as np
import pytest

from deadtrees_amd.data.polygons import PolygonSet, rasterize_host
from deadtrees_amd.deployment.analysis import MapAnalysis, run_host
from deadtrees_amd.deployment.outlines import outlines_from_labels
from deadtrees_amd.deployment.overlaps import PatchOverlaps, overlap_pairs_host
from deadtrees_amd.deployment.patches import PatchConfig, labelled_patches_host
from deadtrees_amd.deployment.stats import RasterStats, zonal_counts_host
from deadtrees_amd.deployment.tiler import Tiler, infer_rasters, infer_tile

K = 3
H, W = 40, 50
OK = np.zeros((H, W), np.uint8)
ZONES = (np.arange(W)[None, :] // 20 + np.zeros((H, 1), int)).astype(np.uint8)             # 0..2


def _square(y, x, r):
    return [(x - r, y - r), (x + r, y - r), (x + r, y + r), (x - r, y + r)]


# (what, the options as infer_tile takes them, a fragment of the message)
BAD = [
    ("zones without stats", dict(zones=ZONES), "stats=True"),
    ("n_zones without stats", dict(n_zones=1), "stats=True"),
    ("patches without stats", dict(patches=True), "stats=True"),
    ("a patch configuration without stats", dict(patches=PatchConfig(4, 2)), "stats=True"),
    ("against without stats", dict(against=OK), "stats=True"),
    ("against_patches without stats", dict(against_patches=PatchConfig()), "stats=True"),
    ("outlines without patches", dict(stats=True, outlines=True), "outlines need patches"),
    ("outlines without patches or stats", dict(outlines=True), "outlines need patches"),
    ("against without patches", dict(stats=True, against=OK), "against needs patches"),
    ("against_patches without against", dict(stats=True, patches=True, against_patches=PatchConfig()), "needs against"),
    ("zones off the grid", dict(stats=True, zones=ZONES[:, :-1]), "grid"),
    ("zones with a third axis", dict(stats=True, zones=ZONES[None]), "grid"),
    ("zones not uint8", dict(stats=True, zones=ZONES.astype(np.int64)), "uint8"),
    ("a zone value above n_zones", dict(stats=True, zones=ZONES, n_zones=2), "smaller"),
    ("a zone value above 7", dict(stats=True, zones=(ZONES + 7).astype(np.uint8)), "n_zones"),
    ("polygon zones above 7", dict(stats=True, zones=PolygonSet.from_polygons([(9, _square(9, 9, 4))])), "n_zones"),
    ("n_zones of 9", dict(stats=True, zones=ZONES, n_zones=9), "n_zones"),
    ("n_zones of 0", dict(stats=True, zones=ZONES, n_zones=0), "n_zones"),
    ("n_zones without zones", dict(stats=True, n_zones=2), "n_zones"),
    ("against off the grid", dict(stats=True, patches=True, against=OK[:, :-1]), "grid"),
    ("against not uint8", dict(stats=True, patches=True, against=OK.astype(np.int32)), "uint8"),
    ("an against value of K", dict(stats=True, patches=True, against=OK + K), "out of range"),
    ("an against polygon of value K", dict(stats=True, patches=True,
                                            against=PolygonSet.from_polygons([(K, _square(9, 9, 4))])), "out of range"),
    ("outlines that are no bool", dict(stats=True, patches=True, outlines="yes"), "outlines"),
    ("patches that are no PatchConfig", dict(stats=True, patches="all"), "PatchConfig"),
    ("against_patches that are no PatchConfig", dict(stats=True, patches=True, against=OK, against_patches=8), "PatchConfig"),
]
IDS = [what.replace(" ", "-") for what, _, _ in BAD]


class _NeverRuns:
    """an inference object that only says how many classes it has"""
    classes = K

    def __getattr__(self, name):
        if name in ("members", "in_channels"):
            raise AttributeError(name)
        raise AssertionError(f"the model was touched ({name}) before the options were checked")


@pytest.mark.parametrize("what,options,fragment", BAD, ids=IDS)
def test_every_entry_point_refuses_a_bad_request(what, options, fragment):
    raster = np.zeros((3, H, W), np.uint8)
    with pytest.raises(ValueError, match=fragment):
        MapAnalysis.of("caller", (H, W), K, **{"stats": False, **options})      # infer_tile's default
    with pytest.raises(ValueError, match=fragment):
        infer_tile(_NeverRuns(), raster, device="cpu", **options)
    per_key = {k: ({0: v} if k in ("zones", "against") else v) for k, v in options.items()}
    queue = infer_rasters(_NeverRuns(), [raster], device="cpu", **per_key)
    with pytest.raises(ValueError, match=fragment):
        next(queue)
    if options.get("stats"):                                     # Tiler.stats always computes statistics
        t = Tiler(tile_shape=(64, 64), subtile_shape=(32, 32))
        t.load_array(raster[:1])
        with pytest.raises(ValueError, match=fragment):
            t.stats(classes=K, **{k: v for k, v in options.items() if k != "stats"})


def test_messages_name_their_caller():
    for who in ("infer_tile", "Tiler.stats"):
        with pytest.raises(ValueError, match=f"^{who}: outlines need patches"):
            MapAnalysis.of(who, (H, W), K, outlines=True)
        with pytest.raises(ValueError, match=f"^{who}: the map must be uint8"):
            MapAnalysis.of(who, (H, W), K, patches=True, against=OK.astype(np.int16))
    with pytest.raises(ValueError, match="^infer_rasters: patches need stats=True"):
        next(infer_rasters(_NeverRuns(), [np.zeros((3, H, W), np.uint8)], device="cpu", patches=True))
    with pytest.raises(ValueError, match="classes"):
        MapAnalysis.of("infer_tile", (H, W), None)


def test_a_valid_request_reads_back_by_name():
    assert MapAnalysis.of("caller", (H, W), K, stats=False) is None
    plain = MapAnalysis.of("caller", (H, W), K)
    assert (plain.K, plain.zones, plain.Z, plain.patches, plain.outlines, plain.against, plain.against_patches) == \
        (K, None, 1, None, False, None, None)
    against = OK.copy()
    full = MapAnalysis.of("caller", (H, W), K, zones=ZONES, n_zones=5, patches=PatchConfig(4, 6), outlines=True,
                          against=against, against_patches=PatchConfig(8, 3))
    assert full.K == K and full.zones is ZONES and full.Z == 5 and full.patches == PatchConfig(4, 6)
    assert full.outlines is True and full.against is against and full.against_patches == PatchConfig(8, 3)
    with pytest.raises(AttributeError):
        full.Z = 2                                               # immutable
    # defaults: n_zones from the map, patches=True, against_patches the connectivity of patches without a sieve
    polys = PolygonSet.from_polygons([(2, _square(9, 9, 4))])
    some = MapAnalysis.of("caller", (H, W), K, zones=ZONES, patches=True, against=polys)
    assert some.Z == 3 and some.patches == PatchConfig() and some.against is polys and some.against_patches == PatchConfig(8)
    assert MapAnalysis.of("caller", (H, W), K, patches=PatchConfig(4, 9), against=OK).against_patches == PatchConfig(4)
    assert MapAnalysis.of("caller", (H, W), K, zones=polys).Z == 3
    # the two steps: one set of rules, a request per raster; a raster without a map has no overlaps
    rules = MapAnalysis.rules("caller", K, True, {}, None, True, None, {}, PatchConfig(8, 2))
    a, b = rules.bind("caller", (H, W), ZONES, OK), rules.bind("caller", (H - 1, W), None, None)
    assert (a.Z, a.against_patches, b.Z, b.against, b.against_patches) == (3, PatchConfig(8, 2), 1, None, None)


# ---------------------------------------------------------------------------------------------- the host runner
def blobs(h, w, seed, density=0.08):
    """seeds dilated by a 3 x 3 square, classes 1 and 2 (the maps of tests/test_overlaps_gpu.py)"""
    rng = np.random.default_rng(seed)
    seeds = np.pad(rng.random((h, w)) < density, 1)
    grown = np.zeros((h, w), bool)
    for dy in range(3):
        for dx in range(3):
            grown |= seeds[dy:dy + h, dx:dx + w]
    return (grown * rng.integers(1, 3, (h, w))).astype(np.uint8)


def two_years():
    """(against, map, zones) on 97 x 131: last year's blobs, the same shifted by (1, 2) with one block of class 2, and three
    zones of 50 columns"""
    a = blobs(97, 131, 21, 0.03)
    b = np.roll(a, (1, 2), (0, 1))
    b[40:60, 40:70] = 2
    return a, b, (np.arange(131)[None, :] // 50 + np.zeros((97, 1), int)).astype(np.uint8)


def composed(result, zones, Z, config, outlines, against, against_config):
    """what ``run_host`` has to return, from the host functions themselves"""
    sieved, labels, table = labelled_patches_host(result, K, config)
    pairs = None
    if against is not None:
        _, labels_a, table_a = labelled_patches_host(against, K, against_config)
        pairs = PatchOverlaps(table_a, table, *overlap_pairs_host(labels_a, labels))
    rings = outlines_from_labels(labels, sieved, config.connectivity) if outlines else None
    return sieved, RasterStats(zonal_counts_host(sieved, zones, K, Z), patches=table, outlines=rings, overlaps=pairs)


@pytest.mark.parametrize("config,patches,rings,pairs", [(PatchConfig(8, 0), 600, 649, 601), (PatchConfig(4, 6), 132, None, 223)])
def test_the_host_runner_is_the_composition_of_the_host_functions(config, patches, rings, pairs):
    a, b, zones = two_years()
    keep = b.copy()
    request = MapAnalysis.of("caller", b.shape, K, zones=zones, patches=config, outlines=True, against=a,
                             against_patches=PatchConfig(8, 3))
    got_map, got = run_host(request, b)
    want_map, want = composed(b, zones, 3, config, True, a, PatchConfig(8, 3))
    assert got == want and got_map.dtype == np.uint8 and np.array_equal(got_map, want_map) and np.array_equal(b, keep)
    # the map is worth the comparison: holes, a sieve that removes and keeps, every class in every zone
    assert got.patches.n == patches and len(got.overlaps) == pairs and (got.counts > 0).all() and got.counts.shape == (3, K)
    assert len(got.outlines) == patches and len(got.outlines.ring_polygon) > patches
    if rings is not None:
        assert len(got.outlines.ring_polygon) == rings and np.array_equal(got_map, b)
    else:
        assert labelled_patches_host(b, K, PatchConfig(4, 0))[2].n == 1007 and not np.array_equal(got_map, b)
    # fewer options: the same figures without the parts that were not asked for
    only = run_host(MapAnalysis.of("caller", b.shape, K, patches=config), b)[1]
    assert only.patches == got.patches and only.outlines is None and only.overlaps is None
    assert np.array_equal(only.counts, got.counts.sum(axis=0, keepdims=True))
    # polygons are burnt with all_touched=True where an array was given
    polys = PolygonSet.from_polygons([(1 + k % 2, _square(10 + 9 * k, 12 + 13 * k, 2.5 + k % 3)) for k in range(9)])
    burnt = rasterize_host(polys, 97, 131, all_touched=True)
    from_polys = run_host(MapAnalysis.of("caller", b.shape, K, zones=polys, patches=config, against=polys), b)[1]
    assert from_polys == run_host(MapAnalysis.of("caller", b.shape, K, zones=burnt, patches=config, against=burnt), b)[1]
    assert len(from_polys.overlaps) > 0 and from_polys.counts.shape == (3, K)
