"""Raster statistics, host layer (deadtrees_amd/deployment/stats.py): ``zonal_counts_host`` against a restatement with
``np.count_nonzero``, the rows / join / forest figures against the reference's rules restated here in numpy
(scripts/computestats_inference.py:16-30,57-75 and scripts/aggregate_results.py:60-81), and ``infer_tile(..., stats=True)``
on the host path with a stub inference object.  All comparisons are exact: integers, or floats computed by the same
operations on the same integers."""
import csv
import functools

import numpy as np
import pytest
import torch

AREA = 0.200022269188281 * 0.200022454940277


@functools.lru_cache(maxsize=None)
def _maps(h, w, K, Z, kind):
    """(classes, zones) uint8 [h, w], seeded; kind "skewed": 97 % class 0, "uniform": all values equally likely"""
    rng = np.random.default_rng(1000 * h + 10 * w + K + 100 * Z + len(kind))
    if kind == "skewed":
        c = np.where(rng.random((h, w)) < 0.97, 0, rng.integers(1, K, (h, w))).astype(np.uint8)
    else:
        c = rng.integers(0, K, (h, w), dtype=np.uint8)
    z = rng.integers(0, Z, (h, w), dtype=np.uint8)
    c.setflags(write=False)
    z.setflags(write=False)
    return c, z


def _count_loop(c, z, K, Z):
    """the independent restatement: one np.count_nonzero per (zone, class)"""
    z = np.zeros_like(c) if z is None else z
    return np.array([[np.count_nonzero((z == zz) & (c == cc)) for cc in range(K)] for zz in range(Z)], dtype=np.int64)


@pytest.mark.parametrize("kind", ["skewed", "uniform"])
@pytest.mark.parametrize("K", [2, 3, 8])
@pytest.mark.parametrize("Z", [1, 3, 8])
@pytest.mark.parametrize("h,w", [(37, 53), (256, 256)])
def test_zonal_counts_host_against_count_nonzero(h, w, K, Z, kind):
    from deadtrees_amd.deployment.stats import zonal_counts_host
    c, z = _maps(h, w, K, Z, kind)
    got = zonal_counts_host(c, z, K, Z)
    assert got.dtype == np.int64 and got.shape == (Z, K)
    assert np.array_equal(got, _count_loop(c, z, K, Z))
    assert int(got.sum()) == h * w
    if Z == 1:
        plain = zonal_counts_host(c, None, K)
        assert plain.shape == (1, K) and np.array_equal(plain, _count_loop(c, None, K, 1))
    if kind == "skewed":
        assert got[:, 0].sum() > 0.95 * h * w
    # a flat view and a non-contiguous one count the same
    assert np.array_equal(zonal_counts_host(c.ravel(), z.ravel(), K, Z), got)
    assert np.array_equal(zonal_counts_host(c[::-1, ::2], z[::-1, ::2], K, Z), _count_loop(c[::-1, ::2], z[::-1, ::2], K, Z))


def test_zonal_counts_host_rejects_values_out_of_range_and_bad_arguments():
    from deadtrees_amd.deployment.stats import zonal_counts_host
    c, z = (a.copy() for a in _maps(37, 53, 3, 3, "uniform"))
    bad = c.copy()
    bad[5, 7] = 3
    with pytest.raises(ValueError, match="class"):
        zonal_counts_host(bad, z, 3, 3)
    with pytest.raises(ValueError, match="class"):
        zonal_counts_host(bad, None, 3, 1)
    badz = z.copy()
    badz[0, 0] = 3
    with pytest.raises(ValueError, match="zone"):
        zonal_counts_host(c, badz, 3, 3)
    for kw in (dict(K=1), dict(K=9), dict(Z=0), dict(Z=9)):
        with pytest.raises(ValueError):
            zonal_counts_host(c, z, **{"K": 3, "Z": 3, **kw})
    with pytest.raises(ValueError, match="zones"):
        zonal_counts_host(c, None, 3, 2)
    with pytest.raises(ValueError, match="shape"):
        zonal_counts_host(c, z[:, :-1], 3, 3)
    with pytest.raises(ValueError, match="uint8"):
        zonal_counts_host(c.astype(np.int64), z, 3, 3)
    with pytest.raises(ValueError, match="uint8"):
        zonal_counts_host(c, z.astype(np.int32), 3, 3)


# ---------------------------------------------------------------------------------------------- computestats_inference
def _reference_row(a, tile):
    """scripts/computestats_inference.py:16-30 and :57-59 restated (np.unique with counts; classes 0, 1, 2)"""
    unique, counts = np.unique(a, return_counts=True)
    row = dict(zip([f"cl_{int(x)}" for x in unique], counts))
    for c in (0, 1, 2):
        if f"cl_{c}" not in row:
            row[f"cl_{c}"] = 0
    row["total"] = int(a.size)
    row["tile"] = tile
    row["deadarea_m2"] = float(np.round((row["cl_1"] + row["cl_2"]) * 0.200022269188281 * 0.200022454940277, 1))
    return row


@pytest.mark.parametrize("case", ["three classes", "no class 2", "two-class model", "with zones"])
def test_stats_row_against_the_reference_rule(case):
    from deadtrees_amd.deployment.stats import RasterStats, stats_row, zonal_counts_host
    K = 2 if case == "two-class model" else 3
    c, z = _maps(256, 256, K, 3, "skewed")
    if case == "no class 2":
        c = np.minimum(c, 1)
    counts = zonal_counts_host(c, z, K, 3) if case == "with zones" else zonal_counts_host(c, None, K)
    got = stats_row(RasterStats(counts), "tile_7")
    want = _reference_row(c, "tile_7")
    assert list(got) == ["tile", "total", "cl_0", "cl_1", "cl_2", "deadarea_m2"]          # always in class order
    assert {k: got[k] for k in want} == {k: (int(v) if k.startswith("cl_") else v) for k, v in want.items()}
    assert set(got) == set(want)
    if case in ("no class 2", "two-class model"):
        assert got["cl_2"] == 0
    assert got["total"] == got["cl_0"] + got["cl_1"] + got["cl_2"] == c.size


def test_raster_stats_properties_and_add():
    from deadtrees_amd.deployment.stats import RasterStats, zonal_counts_host
    c1, z1 = _maps(37, 53, 3, 3, "uniform")
    c2, z2 = _maps(256, 256, 3, 3, "skewed")
    a, b = RasterStats(zonal_counts_host(c1, z1, 3, 3)), RasterStats(zonal_counts_host(c2, z2, 3, 3))
    assert np.array_equal(a.class_counts, [np.count_nonzero(c1 == k) for k in range(3)])
    assert np.array_equal(a.zone_pixels, [np.count_nonzero(z1 == k) for k in range(3)])
    assert a.total == c1.size and a.dead_pixels == np.count_nonzero(c1 >= 1)
    assert a.dead_fraction == np.count_nonzero(c1 >= 1) / c1.size            # server.py:112 on the 0 / 1 map c1 >= 1
    assert a.dead_area_m2 == float(np.round(np.count_nonzero(c1 >= 1) * AREA, 1))
    assert RasterStats(a.counts, pixel_area_m2=1.0).dead_area_m2 == float(a.dead_pixels)
    s = a + b
    both_c, both_z = np.concatenate([c1.ravel(), c2.ravel()]), np.concatenate([z1.ravel(), z2.ravel()])
    assert isinstance(s, RasterStats) and np.array_equal(s.counts, _count_loop(both_c, both_z, 3, 3))
    assert s == RasterStats(zonal_counts_host(both_c, both_z, 3, 3)) and s != a
    assert s.total == a.total + b.total and np.array_equal(a.counts, _count_loop(c1, z1, 3, 3))   # operands unchanged
    assert sum([b], a) == s
    with pytest.raises(ValueError):
        a + RasterStats(zonal_counts_host(c1, None, 3))
    with pytest.raises(ValueError):
        RasterStats(np.zeros(3, np.int64))


def test_merge_years_against_a_literal_table_and_csv_round_trip(tmp_path):
    from deadtrees_amd.deployment.stats import RasterStats, merge_years, stats_row, write_stats_csv

    def row(tile, cl):
        return stats_row(RasterStats(np.array([cl], dtype=np.int64), pixel_area_m2=0.5), tile)

    # tile "b" is missing in the first year, tile "c" in the second
    rows = {2017: [row("a", [90, 7, 3]), row("c", [50, 0, 1])],
            2018: [row("a", [80, 15, 5]), row("b", [196, 3, 1])]}
    table = merge_years(rows)
    columns = ["tile", "total", "cl_0_2017", "cl_1_2017", "cl_2_2017", "deadarea_m2_2017",
               "cl_0_2018", "cl_1_2018", "cl_2_2018", "deadarea_m2_2018"]
    want = [
        dict(zip(columns, ["a", 100, 90, 7, 3, 5.0, 80, 15, 5, 10.0])),
        dict(zip(columns, ["b", None, None, None, None, None, 196, 3, 1, 2.0])),      # total: the FIRST year's, absent
        dict(zip(columns, ["c", 51, 50, 0, 1, 0.5, None, None, None, None])),
    ]
    assert table == want
    assert all(list(r) == columns for r in table)
    # the years' order is the order given
    swapped = merge_years({2018: rows[2018], 2017: rows[2017]})
    assert list(swapped[0])[:3] == ["tile", "total", "cl_0_2018"] and list(swapped[0])[6] == "cl_0_2017"
    assert [r["total"] for r in swapped] == [100, 200, None]
    assert merge_years({}) == []
    with pytest.raises(ValueError):
        merge_years({2017: [row("a", [1, 0, 0]), row("a", [1, 0, 0])]})

    path = tmp_path / "predicted.stats.csv"
    write_stats_csv(path, table)
    with open(path, newline="") as f:
        lines = list(csv.reader(f))
    assert lines[0] == columns
    assert lines[1:] == [["" if r[k] is None else str(r[k]) for k in columns] for r in want]
    assert lines[2][:3] == ["b", "", ""]


# ---------------------------------------------------------------------------------------------- aggregate_results
def _reference_forest(a, b, limit):
    """scripts/aggregate_results.py:60-81 restated: (conifer, broadleaf) or None"""
    res = []
    for c in (1, 2):
        if (b.sum() / b.size) * 100 < limit:
            return None
        dead = a[(a == c) & (b == 1)].sum()
        forest = b.sum()
        res.append((dead / forest) * 100)
    return res


@pytest.mark.parametrize("K", [3, 2])
def test_forest_dead_percent_against_the_reference_rule(K):
    from deadtrees_amd.deployment.stats import RasterStats, forest_dead_percent, zonal_counts_host
    h, w = 100, 100                                    # 10 000 pixels: forest cover in steps of 0.01 %
    rng = np.random.default_rng(5 + K)
    a = rng.integers(0, K, (h, w), dtype=np.uint8)
    for forest_pixels, limit in ((999, 10), (1000, 10), (1001, 10), (2499, 25), (2500, 25), (10000, 10)):
        b = np.zeros(h * w, np.uint8)
        b[rng.permutation(h * w)[:forest_pixels]] = 1
        b = b.reshape(h, w)
        stats = RasterStats(zonal_counts_host(a, b, K, 2))
        want = _reference_forest(a, b, limit)
        got = forest_dead_percent(stats, limit=limit)
        if forest_pixels in (999, 2499):               # just below the limit
            assert want is None and got is None
            continue
        assert want is not None and set(got) == {"conifer", "broadleaf", "total"}
        assert got["conifer"] == want[0] and got["broadleaf"] == want[1] and got["total"] == want[0] + want[1]
        plain = forest_dead_percent(stats, limit=limit, label_weighted=False)
        n1 = np.count_nonzero((a == 1) & (b == 1))
        n2 = np.count_nonzero((a == 2) & (b == 1))
        assert plain["conifer"] == (n1 / forest_pixels) * 100 and plain["broadleaf"] == (n2 / forest_pixels) * 100
        assert got["conifer"] == plain["conifer"]
        assert got["broadleaf"] == ((2 * n2) / forest_pixels) * 100      # the reference sums label values: class 2 doubles
        if K == 2:
            assert got["broadleaf"] == 0 and plain["broadleaf"] == 0
        else:
            assert n2 > 0 and got["broadleaf"] > plain["broadleaf"]
    # another forest zone, and no forest at all
    three = RasterStats(zonal_counts_host(a, (b * 2).astype(np.uint8), K, 3))
    assert forest_dead_percent(three, forest_zone=2) == forest_dead_percent(stats)
    assert forest_dead_percent(three, forest_zone=1, limit=0) is None
    with pytest.raises(ValueError):
        forest_dead_percent(stats, forest_zone=2)


# ---------------------------------------------------------------------------------------------- infer_tile, host path
class _Stub:
    """a 3-class 'network': thresholds of band 0, per sub-tile batch like PyTorchInference.run_u8"""
    classes = 3

    def run_u8(self, u8, device="cpu"):
        return (u8[..., 0] > 250).to(torch.uint8) + (u8[..., 0] > 253).to(torch.uint8)


def _raster(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (4, h, w), dtype=np.uint8)


def test_infer_tile_host_path_returns_the_counts_of_its_map():
    from deadtrees_amd.deployment.stats import RasterStats, zonal_counts_host
    from deadtrees_amd.deployment.tiler import infer_tile
    h, w = 300, 470
    raster = _raster(h, w, 3)
    zones = np.random.default_rng(4).integers(0, 3, (h, w), dtype=np.uint8)
    kw = dict(subtile=64, batch_size=7, device="cpu", on_device=False)
    base = infer_tile(_Stub(), raster, **kw)
    assert isinstance(base, np.ndarray) and base.shape == (h, w) and set(np.unique(base)) == {0, 1, 2}
    got, stats = infer_tile(_Stub(), raster, stats=True, zones=zones, **kw)
    assert np.array_equal(got, base) and got.dtype == base.dtype
    assert isinstance(stats, RasterStats) and np.array_equal(stats.counts, zonal_counts_host(base, zones, 3, 3))
    got, plain = infer_tile(_Stub(), raster, stats=True, **kw)
    assert np.array_equal(got, base) and plain.counts.shape == (1, 3)
    assert np.array_equal(plain.counts, zonal_counts_host(base, None, 3))
    assert np.array_equal(plain.class_counts, stats.class_counts)
    _, wide = infer_tile(_Stub(), raster, stats=True, zones=zones, n_zones=8, **kw)
    assert wide.counts.shape == (8, 3) and np.array_equal(wide.counts[:3], stats.counts) and not wide.counts[3:].any()
    # a previous map as zones: the transition matrix
    prev = np.roll(base, 5, axis=1)
    _, trans = infer_tile(_Stub(), raster, stats=True, zones=prev, n_zones=3, **kw)
    for a in range(3):
        for b in range(3):
            assert trans.counts[a, b] == np.count_nonzero((prev == a) & (base == b))
    # a blank raster is still None
    blank = raster.copy()
    blank[0] = np.where(blank[0] > 127, 255, 0)
    assert infer_tile(_Stub(), blank, stats=True, zones=zones, skip_blank=True, **kw) is None


def test_infer_tile_validates_the_stats_arguments_before_any_work():
    from deadtrees_amd.deployment.tiler import infer_rasters, infer_tile

    class _Never(_Stub):
        def run_u8(self, *a, **k):
            raise AssertionError("validation must come first")

        run_blocks = run_windows = run_u8

    class _NoClasses:
        run_u8 = _Never.run_u8

    h, w = 100, 130
    raster = _raster(h, w)
    zones = np.random.default_rng(1).integers(0, 3, (h, w), dtype=np.uint8)
    kw = dict(subtile=64, device="cpu", on_device=False)
    with pytest.raises(ValueError, match="stats"):
        infer_tile(_Never(), raster, zones=zones, **kw)                           # zones without stats
    with pytest.raises(ValueError, match="grid"):
        infer_tile(_Never(), raster, stats=True, zones=zones[:, :-1], **kw)       # wrong shape
    with pytest.raises(ValueError, match="grid"):
        infer_tile(_Never(), raster, stats=True, zones=zones[None], **kw)
    with pytest.raises(ValueError, match="uint8"):
        infer_tile(_Never(), raster, stats=True, zones=zones.astype(np.int64), **kw)
    for n_zones in (0, 9, -1):
        with pytest.raises(ValueError, match="n_zones"):
            infer_tile(_Never(), raster, stats=True, zones=zones, n_zones=n_zones, **kw)
    with pytest.raises(ValueError, match="smaller"):
        infer_tile(_Never(), raster, stats=True, zones=zones, n_zones=2, **kw)
    with pytest.raises(ValueError, match="n_zones"):
        infer_tile(_Never(), raster, stats=True, zones=(zones + 7).astype(np.uint8), **kw)   # zones.max() + 1 = 10 > 8
    with pytest.raises(ValueError, match="classes"):
        infer_tile(_NoClasses(), raster, stats=True, **kw)
    # the device paths check first as well (no GPU is touched: the stub would raise)
    for extra in (dict(overlap=16), dict(overlap=16, blend="average"), dict(tta="flips"), dict()):
        with pytest.raises(ValueError, match="stats"):
            infer_tile(_Never(), raster, subtile=64, zones=zones, **extra)
        with pytest.raises(ValueError, match="smaller"):
            infer_tile(_Never(), raster, subtile=64, stats=True, zones=zones, n_zones=1, **extra)
    with pytest.raises(ValueError, match="stats"):
        list(infer_rasters(_Never(), [raster], zones={0: zones}, subtile=64, device="cpu"))


def test_infer_rasters_host_path_with_zones_by_key():
    from deadtrees_amd.deployment.stats import zonal_counts_host
    from deadtrees_amd.deployment.tiler import infer_rasters, infer_tile
    rasters = [("a", _raster(100, 130, 1)), ("b", _raster(64, 64, 2)), ("c", _raster(70, 90, 3))]
    zones = {key: np.random.default_rng(9).integers(0, 2, arr.shape[1:], dtype=np.uint8) for key, arr in rasters}
    kw = dict(subtile=64, device="cpu", stats=True)
    by_map = dict(infer_rasters(_Stub(), rasters, zones=zones, n_zones=2, **kw))
    by_call = dict(infer_rasters(_Stub(), rasters, zones=lambda key: zones[key], n_zones=2, **kw))
    some = dict(infer_rasters(_Stub(), rasters, zones={"a": zones["a"]}, **kw))       # a missing key: no zones
    for key, arr in rasters:
        base = infer_tile(_Stub(), arr, subtile=64, device="cpu")
        for got in (by_map[key], by_call[key]):
            assert np.array_equal(got[0], base)
            assert np.array_equal(got[1].counts, zonal_counts_host(base, zones[key], 3, 2))
        assert np.array_equal(some[key][0], base)
        assert np.array_equal(some[key][1].class_counts, by_map[key][1].class_counts)
        assert some[key][1].counts.shape == ((2, 3) if key == "a" else (1, 3))
    # without stats the pairs are what they were
    assert isinstance(dict(infer_rasters(_Stub(), rasters, subtile=64, device="cpu"))["a"], np.ndarray)


def test_tiler_stats_on_the_reference_loop():
    from deadtrees_amd.deployment.stats import zonal_counts_host
    from deadtrees_amd.deployment.tiler import Tiler
    raster = _raster(300, 470, 6)
    zones = np.random.default_rng(7).integers(0, 3, (300, 470), dtype=np.uint8)
    t = Tiler(tile_shape=(512, 512), subtile_shape=(128, 128))
    with pytest.raises(RuntimeError):
        t.stats()
    t.load_array(raster)
    t.put_batches((t.get_batches()[:, 0] > 200).astype(np.uint8) * 2)             # classes 0 and 2 of a 3-class model
    assert np.array_equal(t.stats().counts, zonal_counts_host(t.result, None, 3))
    assert np.array_equal(t.stats(zones, classes=3, n_zones=3).counts, zonal_counts_host(t.result, zones, 3, 3))
    assert np.array_equal(t.stats(zones).counts, zonal_counts_host(t.result, zones, 3, 3))
    assert t.stats().counts[0, 1] == 0 and t.stats().total == 300 * 470
    with pytest.raises(ValueError):
        t.stats(classes=2)                                                        # the map holds class 2
    with pytest.raises(ValueError):
        t.stats(zones[:-1])


def test_library_rejects_bad_arguments_before_any_launch():
    """``dt_zonal_counts_u8`` checks its arguments on the host (no GPU needed to see the error; the addresses are never
    read)"""
    from deadtrees_amd import _lib
    lib = _lib.load()
    c, z, counts, err = 0x1000, 0x2003, 0x3000, 0x4000
    for args, word in (((c, z, 100, 1, 1, counts, err), b"K=1"), ((c, z, 100, 9, 1, counts, err), b"K=9"),
                       ((c, z, 100, 3, 0, counts, err), b"Z=0"), ((c, z, 100, 3, 9, counts, err), b"Z=9"),
                       ((c, None, 100, 3, 2, counts, err), b"zones"), ((c, z, 0, 3, 3, counts, err), b"n must be"),
                       ((None, z, 100, 3, 3, counts, err), b"null"), ((c, z, 100, 3, 3, None, err), b"null"),
                       ((c, z, 100, 3, 3, counts, None), b"null")):
        assert lib.dt_zonal_counts_u8(*args, None) < 0, args
        assert word in lib.dt_last_error(), (args, lib.dt_last_error())
