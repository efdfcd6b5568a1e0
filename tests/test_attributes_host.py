"""``deployment/attributes.py`` on the CPU: a hand-computed case, the two quantisation rules, ``patch_attributes_host`` against a
plain Python double loop, 64-bit sums, the option's rules from ONE table of bad requests raised alike by every entry point,
``run_host`` against the direct composition, ``Tiler.stats``, an unchanged ``RasterStats`` without the option and the
``properties()`` columns in GeoJSON.  The tables are integers: every comparison of them is exact."""
import numpy as np
import pytest

import test_analysis_host as th
from deadtrees_amd.deployment.analysis import MapAnalysis, run_host
from deadtrees_amd.deployment.attributes import (AttributeConfig, PatchAttributes, attribute_tables_host, confidence_q,
                                                 index_t, patch_attributes, patch_attributes_host, table_columns)
from deadtrees_amd.deployment.outlines import outlines_geojson
from deadtrees_amd.deployment.patches import PatchConfig, labelled_patches_host
from deadtrees_amd.deployment.stats import RasterStats
from deadtrees_amd.deployment.tiler import Tiler, infer_rasters, infer_tile

K = th.K


def random_case(h, w, C, seed, density=0.12):
    """(map uint8 [h, w], raster uint8 [C, h, w], probs fp32 [K, h, w]): blobs, bytes with 0 and 255 among them, a softmax of
    random logits with an exact 0.0 and an exact 1.0 planted on labelled pixels when there are any"""
    rng = np.random.default_rng(seed)
    m = th.blobs(h, w, seed, density)
    raster = rng.integers(0, 256, (C, h, w)).astype(np.uint8)
    raster[:, rng.random((h, w)) < 0.05] = 0              # s == 0 pixels for every pair
    raster[rng.random((C, h, w)) < 0.05] = 255
    logits = rng.normal(0, 2, (K, h, w)).astype(np.float32)
    e = np.exp(logits - logits.max(axis=0))
    probs = (e / e.sum(axis=0)).astype(np.float32)
    ys, xs = np.nonzero(m)
    if len(ys) >= 2:
        probs[m[ys[0], xs[0]], ys[0], xs[0]] = 0.0
        probs[m[ys[-1], xs[-1]], ys[-1], xs[-1]] = 1.0
    return m, raster, probs


def loop(labels, table, raster, classes, probs, pairs):
    """the contract as a plain Python double loop: the dictionary of arrays a ``PatchAttributes`` holds"""
    C, n = len(raster), table.n
    row_of = {int(r): k for k, r in enumerate(table.root)}
    out = dict(band_sum=np.zeros((n, C), np.int64), band_sumsq=np.zeros((n, C), np.int64),
               band_min=np.full((n, C), 255, np.uint8), band_max=np.zeros((n, C), np.uint8),
               index_sum=np.zeros((n, len(pairs)), np.int64), conf_sum=np.zeros(n, np.int64),
               conf_min=np.full(n, 65535, np.int32))
    for y in range(labels.shape[0]):
        for x in range(labels.shape[1]):
            if labels[y, x] == 0:
                continue
            r = row_of[int(labels[y, x]) - 1]
            v = [int(raster[c, y, x]) for c in range(C)]
            for c in range(C):
                out["band_sum"][r, c] += v[c]
                out["band_sumsq"][r, c] += v[c] * v[c]
                out["band_min"][r, c] = min(out["band_min"][r, c], v[c])
                out["band_max"][r, c] = max(out["band_max"][r, c], v[c])
            for k, (a, b) in enumerate(pairs):
                s = v[a] + v[b]
                out["index_sum"][r, k] += (v[a] * 65534 + s // 2) // s if s else 32767
            if probs is not None:
                p = np.float32(probs[classes[y, x], y, x])
                p = p if p > 0 else np.float32(0)
                p = min(p, np.float32(1))
                q = int(np.floor(np.float32(np.float32(p * np.float32(65535)) + np.float32(0.5))))
                out["conf_sum"][r] += q
                out["conf_min"][r] = min(out["conf_min"][r], q)
    return out


def same(attrs: PatchAttributes, want: dict, confidence: bool):
    for name, array in want.items():
        if name.startswith("conf") and not confidence:
            assert getattr(attrs, name) is None
            continue
        got = getattr(attrs, name)
        assert got.dtype == array.dtype and np.array_equal(got, array), name


# ---------------------------------------------------------------------------------------------- the contract
def test_hand_computed_case():
    m = np.array([[1, 1, 0, 0, 0],
                  [1, 0, 0, 2, 2],
                  [0, 0, 0, 2, 0],
                  [0, 0, 0, 0, 0]], np.uint8)
    raster = np.zeros((2, 4, 5), np.uint8)
    raster[0, :2] = [[10, 20, 1, 1, 1], [30, 1, 1, 0, 200]]
    raster[0, 2, 3] = 100
    raster[1, :2] = [[10, 0, 7, 7, 7], [90, 7, 7, 0, 200]]
    raster[1, 2, 3] = 50
    probs = np.zeros((3, 4, 5), np.float32)
    probs[1, 0, 0], probs[1, 0, 1], probs[1, 1, 0] = 0.5, 1.0, 0.25
    probs[2, 1, 3], probs[2, 1, 4], probs[2, 2, 3] = 0.75, np.nan, 2.0
    _, labels, table = labelled_patches_host(m, K, PatchConfig(4))
    assert table.root.tolist() == [0, 8] and table.area.tolist() == [3, 3]
    a = patch_attributes_host(labels, table, raster, m, probs, AttributeConfig(((0, 1),), confidence=True))
    assert a.band_sum.tolist() == [[60, 100], [300, 250]]
    assert a.band_sumsq.tolist() == [[1400, 8200], [50000, 42500]]
    assert a.band_min.tolist() == [[10, 0], [0, 0]] and a.band_max.tolist() == [[30, 90], [200, 200]]
    # t: 10/20 -> 32767, 20/20 -> 65534, 30/120 -> (30 * 65534 + 60) // 120 = 16384; 0/0 -> 32767, 200/400 -> 32767,
    # 100/150 -> (6553400 + 75) // 150 = 43689
    assert a.index_sum.tolist() == [[32767 + 65534 + 16384], [32767 + 32767 + 43689]]
    # q: 0.5 -> floor(32767.5 + 0.5) = 32768, 1.0 -> 65535, 0.25 -> floor(16383.75 + 0.5) = 16384; 0.75 -> 49151.25 + 0.5 ->
    # 49151, NaN -> 0, 2.0 -> 65535
    assert a.conf_sum.tolist() == [32768 + 65535 + 16384, 49151 + 0 + 65535] and a.conf_min.tolist() == [16384, 0]
    assert np.allclose(a.mean(), [[20, 100 / 3], [100, 250 / 3]]) and a.mean().dtype == np.float64
    assert np.allclose(a.std(), np.sqrt([[1400 / 3 - 400, 8200 / 3 - (100 / 3) ** 2],
                                         [50000 / 3 - 10000, 42500 / 3 - (250 / 3) ** 2]]))
    assert np.allclose(a.index(0), [((32767 + 65534 + 16384) / 3 - 32767) / 32767, ((2 * 32767 + 43689) / 3 - 32767) / 32767])
    assert np.allclose(a.confidence(), [(0.5 + 1 + 0.25) / 3, (0.75 + 0 + 1) / 3], atol=1e-5)
    assert np.allclose(a.min_confidence(), [0.25, 0.0], atol=1e-5)
    assert a == patch_attributes_host(labels, table, raster, m, probs, AttributeConfig([(0, 1)], True))
    assert a != patch_attributes_host(labels, table, raster, m, probs, AttributeConfig(((1, 0),), True)) and a != "a"
    plain = patch_attributes_host(labels, table, raster)
    assert plain != a and plain.indices == () and plain.conf_sum is None and not plain.has_confidence
    assert repr(plain) == "PatchAttributes(n=2, bands=2, indices=[], confidence=False)"
    assert repr(a) == "PatchAttributes(n=2, bands=2, indices=[(0, 1)], confidence=True, weakest mean confidence 0.583)"
    with pytest.raises(ValueError, match="confidence"):
        plain.confidence()
    with pytest.raises(ValueError, match="index"):
        plain.index(0)


def test_quantisation_rules():
    q = confidence_q(np.array([0.0, 1.0, np.nan, 1.0 + 1e-6, -0.5, np.inf, -np.inf], np.float32))
    assert q.tolist() == [0, 65535, 0, 65535, 0, 65535, 0]
    assert int(index_t(0, 0)) == 32767 and int(index_t(255, 0)) == 65534 and int(index_t(0, 255)) == 0
    assert int(index_t(255, 255)) == 32767 and int(index_t(1, 1)) == 32767
    # t is round(65534 * a / s) for every pair of bytes, and stays in [0, 65534]
    a, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    t = index_t(a.astype(np.uint8), b.astype(np.uint8))
    s = np.maximum(a + b, 1)
    assert t.min() == 0 and t.max() == 65534
    assert np.array_equal(t[1:, 1:], np.floor(65534 * a[1:, 1:] / s[1:, 1:] + 0.5).astype(np.int64))
    # the product and the sum are float32 roundings: 0.7 * 65535 is no float64 computation
    p = np.float32(0.7)
    assert int(confidence_q(p)) == int(np.floor(np.float32(np.float32(p * np.float32(65535)) + np.float32(0.5))))


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("min_pixels", [0, 4])
def test_host_equals_a_plain_loop(connectivity, min_pixels):
    m, raster, probs = random_case(37, 53, 4, 5)
    pairs = ((3, 0), (1, 2), (0, 0), (2, 3))
    sieved, labels, table = labelled_patches_host(m, K, PatchConfig(connectivity, min_pixels))
    assert table.n > 20 and (table.area > 1).any() and ((sieved != m).any() == (min_pixels > 0))
    want = loop(labels, table, raster, sieved, probs, pairs)
    same(patch_attributes_host(labels, table, raster, sieved, probs, AttributeConfig(pairs, True)), want, True)
    assert want["conf_sum"].max() > 65535 and (want["index_sum"][:, 2] == 32767 * table.area).all()    # pair (0, 0): t = 32767
    # the default: NDVI alone, no confidence without probabilities, confidence with them
    default = patch_attributes_host(labels, table, raster)
    assert default.indices == ((3, 0),) and np.array_equal(default.index_sum[:, 0], want["index_sum"][:, 0])
    same(default, {k: v for k, v in want.items() if k != "index_sum"}, False)
    assert patch_attributes_host(labels, table, raster, sieved, probs).has_confidence
    # maps in: the same from the class map, unsieved classes included (only labelled pixels are read)
    got = patch_attributes(m, raster, K, probs, PatchConfig(connectivity, min_pixels), AttributeConfig(pairs, True))
    same(got, want, True)
    assert got.table == table
    # a subset of the roots, and a root without pixels
    sums, ext = attribute_tables_host(labels, table.root[::3], raster, sieved, probs, pairs)
    full = attribute_tables_host(labels, table.root, raster, sieved, probs, pairs)
    assert np.array_equal(sums, full[0][::3]) and np.array_equal(ext, full[1][::3])
    free = int(np.flatnonzero(labels.ravel() == 0)[0])
    sums, ext = attribute_tables_host(labels, [free], raster, sieved, probs, pairs[:1])
    assert sums.tolist() == [[0] * 10] and ext.tolist() == [[255] * 4 + [0] * 4 + [65535]]


def test_sums_are_64_bit():
    m = np.ones((300, 300), np.uint8)
    _, labels, table = labelled_patches_host(m, K, PatchConfig())
    a = patch_attributes_host(labels, table, np.full((1, 300, 300), 255, np.uint8))
    assert table.n == 1 and a.band_sumsq.tolist() == [[5_852_250_000]] and a.band_sum.tolist() == [[22_950_000]]
    assert a.mean().tolist() == [[255.0]] and a.std().tolist() == [[0.0]]


def test_bad_arguments_of_the_host_functions():
    m, raster, probs = random_case(9, 11, 3, 2)
    _, labels, table = labelled_patches_host(m, K, PatchConfig())
    for bad, fragment in ((dict(labels=labels.astype(np.int64)), "int32"), (dict(raster=raster.astype(np.int16)), "uint8"),
                          (dict(raster=raster[:, :-1]), "grid"), (dict(raster=np.zeros((9, 9, 11), np.uint8)), "C <= 8"),
                          (dict(indices=((0, 3),)), "band"), (dict(probs=probs), "class map"),
                          (dict(probs=probs.astype(np.float64), classes=m), "float32"),
                          (dict(probs=probs[:, :-1], classes=m), "float32"), (dict(probs=probs[:2], classes=m), "out of range"),
                          (dict(probs=probs, classes=m.astype(np.int32)), "uint8")):
        with pytest.raises(ValueError, match=fragment):
            attribute_tables_host(**{**dict(labels=labels, roots=table.root, raster=raster), **bad})
    for bad in (dict(indices=((0, 1),) * 5), dict(indices=((0, 8),)), dict(indices=((0, 1.5),)), dict(indices=(3,)),
                dict(indices=7), dict(confidence="yes")):
        with pytest.raises(ValueError, match="AttributeConfig"):
            AttributeConfig(**bad)
    assert AttributeConfig() == AttributeConfig(None, False) != AttributeConfig(()) and AttributeConfig().pairs(3) == ()
    assert AttributeConfig().pairs(4) == ((3, 0),) and AttributeConfig([[1, 0]]).pairs(2) == ((1, 0),)
    assert repr(AttributeConfig(((3, 0),), True)) == "AttributeConfig(indices=((3, 0),), confidence=True)"
    assert table_columns(4, 1, True) == (10, 9) and table_columns(3, 0, False) == (6, 6)
    with pytest.raises(ValueError, match="expected tables"):
        PatchAttributes(table, np.zeros((table.n, 5)), np.zeros((table.n, 6)), 3)
    with pytest.raises(ValueError, match="confidence needs"):
        patch_attributes(m, raster, K, config=AttributeConfig(confidence=True))
    with pytest.raises(ValueError, match="AttributeConfig"):
        patch_attributes(m, raster, K, config=True)


# ---------------------------------------------------------------------------------------------- the option's rules
RGBN = np.zeros((4, th.H, th.W), np.uint8)
AVERAGE = dict(overlap=16, blend="average", subtile=64)
# (what, the options as infer_tile takes them, the raster, a fragment of the message, entry points that take the case)
BAD = [
    ("attributes without stats", dict(attributes=True), RGBN, "attributes need stats=True", "all"),
    ("a configuration without stats", dict(attributes=AttributeConfig(())), RGBN, "attributes need stats=True", "all"),
    ("attributes without patches", dict(stats=True, attributes=True), RGBN, "attributes need patches", "all"),
    ("attributes of a wrong type", dict(stats=True, patches=True, attributes="ndvi"), RGBN, "attributes must be", "all"),
    ("attributes that are a PatchConfig", dict(stats=True, patches=True, attributes=PatchConfig()), RGBN,
     "attributes must be", "all"),
    ("a band the raster lacks", dict(stats=True, patches=True, attributes=AttributeConfig(((4, 0),))), RGBN, "band", "all"),
    ("NDVI of three bands", dict(stats=True, patches=True, attributes=AttributeConfig(((3, 0),))), RGBN[:3], "band", "all"),
    ("a raster that is not uint8", dict(stats=True, patches=True, attributes=True), RGBN.astype(np.int16), "uint8", "all"),
    ("nine bands", dict(stats=True, patches=True, attributes=True), np.zeros((9, th.H, th.W), np.uint8), "C <= 8", "all"),
    ("confidence on the block path", dict(stats=True, patches=True, attributes=AttributeConfig(confidence=True)), RGBN,
     "need probabilities", "all"),
    ("confidence under blend=crop", dict(stats=True, patches=True, attributes=AttributeConfig(confidence=True), overlap=16,
                                         subtile=64), RGBN, "need probabilities .*blend='average'", "infer"),
    ("confidence under tta and crop", dict(stats=True, patches=True, attributes=AttributeConfig(confidence=True),
                                           tta="flips"), RGBN, "need probabilities .*blend='average'", "infer"),
]


class _HardVote(th._NeverRuns):
    """an ensemble that votes hard and must not be touched beyond that"""
    members, vote = (th._NeverRuns(), th._NeverRuns()), "hard"


@pytest.mark.parametrize("what,options,raster,fragment,where", BAD, ids=[b[0].replace(" ", "-") for b in BAD])
def test_every_entry_point_refuses_a_bad_request(what, options, raster, fragment, where):
    path = {k: v for k, v in options.items() if k in ("overlap", "blend", "subtile", "tta")}
    plain = {k: v for k, v in options.items() if k not in path}
    if where == "all":
        for who in ("caller", "Tiler.stats"):
            with pytest.raises(ValueError, match=f"^{who}: .*{fragment}"):
                MapAnalysis.of(who, (th.H, th.W), K, raster=raster, **{"stats": False, **plain},
                               no_probs="this caller has none")
    with pytest.raises(ValueError, match=f"^infer_tile: .*{fragment}"):
        infer_tile(th._NeverRuns(), raster, device="cpu", **options)           # before the model is touched
    queue = infer_rasters(th._NeverRuns(), [raster], device="cpu", **options)
    with pytest.raises(ValueError, match=f"^infer_(rasters|tile): .*{fragment}"):
        next(queue)                                                            # at the first next()
    if where == "all" and options.get("stats"):
        t = Tiler(tile_shape=(64, 64), subtile_shape=(32, 32))
        t.load_array(raster)
        with pytest.raises(ValueError, match=f"^Tiler.stats: .*{fragment}"):
            t.stats(classes=K, **{k: v for k, v in plain.items() if k != "stats"})


def test_confidence_is_accepted_where_return_probs_is():
    confident = dict(stats=True, patches=True, attributes=AttributeConfig(confidence=True))
    with pytest.raises(ValueError, match="^infer_tile: attributes with confidence=True need probabilities .*vote='soft'"):
        infer_tile(_HardVote(), RGBN, device="cpu", **AVERAGE, **confident)
    with pytest.raises(ValueError, match="^infer_tile: return_probs needs blend='average'"):
        infer_tile(_HardVote(), RGBN, device="cpu", return_probs=True, **AVERAGE)
    # on the average path the request is valid: the rules pass and the model is what gets touched next
    with pytest.raises((AssertionError, ValueError), match="touched|run_windows"):
        infer_tile(th._NeverRuns(), RGBN, device="cpu", **AVERAGE, **confident)
    request = MapAnalysis.of("caller", (th.H, th.W), K, raster=RGBN, patches=True, attributes=AttributeConfig(confidence=True))
    assert request.attributes == AttributeConfig(((3, 0),), True)               # bound: the pairs are written out
    assert MapAnalysis.of("caller", (th.H, th.W), K, raster=RGBN[:3], patches=True, attributes=True).attributes.indices == ()
    assert MapAnalysis.of("caller", (th.H, th.W), K, patches=True).attributes is None
    assert MapAnalysis.of("caller", (th.H, th.W), K, patches=True, attributes=False, raster=None).attributes is None
    with pytest.raises(ValueError, match="^caller: attributes need the raster"):
        MapAnalysis.of("caller", (th.H, th.W), K, patches=True, attributes=True)
    with pytest.raises(ValueError, match="^caller: .*grid"):
        MapAnalysis.of("caller", (th.H, th.W), K, raster=RGBN[:, 1:], patches=True, attributes=True)
    # the positional order of the rules is the parent's, with the new options behind it
    rules = MapAnalysis.rules("caller", K, True, None, None, True, None, None, None, None, None, True)
    assert rules.attributes == AttributeConfig() and rules.bind("caller", (th.H, th.W), raster=RGBN).attributes.indices == ((3, 0),)


# ---------------------------------------------------------------------------------------------- the runners
def test_the_host_runner_is_the_composition_of_the_host_functions():
    a, b, zones = th.two_years()
    _, raster, probs = random_case(97, 131, 4, 9)
    raster.setflags(write=False)
    config, attributes = PatchConfig(4, 6), AttributeConfig(((3, 0), (1, 2)), confidence=True)
    options = dict(zones=zones, patches=config, outlines=True, against=a, against_patches=PatchConfig(8, 3), gaps=True)
    plain_map, plain = run_host(MapAnalysis.of("caller", b.shape, K, **options), b)
    request = MapAnalysis.of("caller", b.shape, K, raster=raster, attributes=attributes, **options)
    full_map, full = run_host(request, b, raster=raster, probs=probs)
    sieved, labels, table = labelled_patches_host(b, K, config)
    want = patch_attributes_host(labels, table, raster, sieved, probs, attributes)
    assert full.attributes == want and want.table == full.patches and table.n == 132 and not np.array_equal(sieved, b)
    same(full.attributes, loop(labels, table, raster, sieved, probs, attributes.indices), True)
    # everything else is what the call without the option returns
    assert np.array_equal(full_map, plain_map) and full != plain and plain.attributes is None
    assert RasterStats(full.counts, patches=full.patches, outlines=full.outlines, overlaps=full.overlaps, gaps=full.gaps) == plain
    only = run_host(MapAnalysis.of("caller", b.shape, K, raster=raster, patches=config, attributes=True), b, raster=raster)[1]
    assert only.attributes == patch_attributes_host(labels, table, raster) and only.gaps is None and only.overlaps is None


def test_raster_stats_without_the_option_are_the_parents():
    a, b, zones = th.two_years()
    _, raster, _ = random_case(97, 131, 4, 9)
    options = dict(zones=zones, patches=PatchConfig(8), gaps=True)
    plain = run_host(MapAnalysis.of("caller", b.shape, K, **options), b)[1]
    full = run_host(MapAnalysis.of("caller", b.shape, K, raster=raster, attributes=True, **options), b, raster=raster)[1]
    assert "attributes" not in repr(plain) and repr(plain).endswith(f", gaps={plain.gaps!r})")
    assert repr(full) == repr(plain)[:-1] + f", attributes={full.attributes!r})"
    assert "attributes=PatchAttributes(n=600, bands=4, indices=[(3, 0)], confidence=False)" in repr(full)
    again = RasterStats(plain.counts, patches=plain.patches, gaps=plain.gaps)
    assert again == plain and repr(again) == repr(plain) and again.attributes is None and plain != full and full != plain
    assert RasterStats(full.counts, patches=full.patches, gaps=full.gaps, attributes=full.attributes) == full
    total = full + full
    assert total.attributes is None and total.patches is None and total == plain + plain
    assert repr(total) == repr(plain + plain)
    with pytest.raises(ValueError, match="attributes"):
        RasterStats(plain.counts, attributes=full.attributes)
    with pytest.raises(ValueError, match="attributes"):
        RasterStats(plain.counts, patches=plain.patches, attributes="all")
    other = labelled_patches_host(a, K, PatchConfig(8))
    with pytest.raises(ValueError, match="attributes"):
        RasterStats(plain.counts, patches=plain.patches, attributes=patch_attributes_host(other[1], other[2], raster))


def test_tiler_stats_reads_its_loaded_raster():
    m, raster, _ = random_case(th.H, th.W, 4, 3)
    t = Tiler(tile_shape=(64, 64), subtile_shape=(32, 32))
    t.load_array(raster)
    t.result[...] = m
    config = PatchConfig(8, 3)
    stats = t.stats(classes=K, patches=config, attributes=True)
    sieved, labels, table = labelled_patches_host(m, K, config)
    assert stats.attributes == patch_attributes_host(labels, table, raster) and stats.attributes.indices == ((3, 0),)
    assert np.array_equal(t.result, sieved) and stats.patches == table and table.n > 5
    assert t.stats(classes=K, patches=config).attributes is None
    pairs = t.stats(classes=K, patches=config, attributes=AttributeConfig(((0, 1), (2, 3)))).attributes
    assert pairs.indices == ((0, 1), (2, 3)) and pairs.index_sum.shape == (table.n, 2)
    # the host path of infer_tile: a model that returns a fixed map
    class Fixed:
        classes, in_channels = K, 4

        def run_u8(self, u8, device=None):
            import torch
            assert u8.shape[-1] == 4
            return torch.from_numpy(np.ascontiguousarray(m[None, :32, :32])).expand(len(u8), 32, 32)
    got_map, got = infer_tile(Fixed(), raster, subtile=32, device="cpu", stats=True, patches=True, attributes=True)
    _, labels, table = labelled_patches_host(got_map, K, PatchConfig())
    assert got.attributes == patch_attributes_host(labels, table, raster) and table.n > 0


def test_properties_reach_the_geojson_features():
    m, raster, probs = random_case(37, 53, 4, 5)
    request = MapAnalysis.of("caller", m.shape, K, raster=raster, patches=PatchConfig(8, 4), outlines=True,
                             attributes=AttributeConfig(((3, 0), (1, 2)), True))
    stats = run_host(request, m, raster=raster, probs=probs)[1]
    a = stats.attributes
    columns = a.properties()
    assert list(columns) == ([f"{s}_b{c}" for c in range(4) for s in ("mean", "std", "min", "max")]
                             + ["ndvi", "nd_1_2", "confidence", "min_confidence"])
    assert all(len(v) == stats.patches.n for v in columns.values())
    assert np.array_equal(columns["ndvi"], a.index(0)) and np.array_equal(columns["min_b2"], a.band_min[:, 2])
    assert list(a.properties(["confidence", "ndvi"])) == ["confidence", "ndvi"]
    with pytest.raises(ValueError, match="no column 'median_b0'"):
        a.properties(["median_b0"])
    doc = outlines_geojson(stats.outlines, table=stats.patches, properties=a.properties())
    assert len(doc["features"]) == stats.patches.n > 10
    for k in (0, stats.patches.n - 1):
        props = doc["features"][k]["properties"]
        assert props["ndvi"] == float(a.index(0)[k]) and props["max_b3"] == int(a.band_max[k, 3])
        assert props["confidence"] == float(a.confidence()[k]) and isinstance(props["min_b0"], int)
        assert -1.0 <= props["ndvi"] <= 1.0 and 0.0 <= props["min_confidence"] <= props["confidence"] <= 1.0
    assert "ndvi" not in patch_attributes_host(*labelled_patches_host(m, K, PatchConfig())[1:], raster[:3]).properties()
