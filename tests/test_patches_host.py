"""Dead-tree patches on the host (``deployment/patches.py``): the contract the device path is compared against.  No GPU.

``label_patches_host`` against answers written out by hand and against a breadth-first flood fill written here;
``measure_patches_host`` against a per-patch ``np.nonzero``; ``sieve_host``; the ``PatchTable`` helpers; every
``ValueError``; ``RasterStats(patches=...)``; ``Tiler.stats(patches=...)``.  Integers only: every comparison is exact."""
from collections import deque

import numpy as np
import pytest

from deadtrees_amd.deployment.patches import (PatchConfig, PatchTable, check_patches, label_patches_host,
                                              measure_patches_host, patches_host, sieve_host)
from deadtrees_amd.deployment.stats import PIXEL_AREA_M2, RasterStats, zonal_counts_host


def _u8(rows):
    return np.array(rows, dtype=np.uint8)


def _flood(classes, K, connectivity):
    """brute force: breadth-first from every unlabelled pixel in row-major order, so the seed is the patch's first pixel"""
    h, w = classes.shape
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)]
    if connectivity == 8:
        steps += [(-1, -1), (-1, 1), (1, -1), (1, 1)]
    labels = np.zeros((h, w), np.int32)
    for y0 in range(h):
        for x0 in range(w):
            c = classes[y0, x0]
            if c == 0 or c >= K or labels[y0, x0]:
                continue
            labels[y0, x0] = y0 * w + x0 + 1
            todo = deque([(y0, x0)])
            while todo:
                y, x = todo.popleft()
                for dy, dx in steps:
                    qy, qx = y + dy, x + dx
                    if 0 <= qy < h and 0 <= qx < w and classes[qy, qx] == c and not labels[qy, qx]:
                        labels[qy, qx] = y0 * w + x0 + 1
                        todo.append((qy, qx))
    return labels


# ---------------------------------------------------------------------------------------------- labels
def test_labels_of_a_5x7_map_written_out_by_hand():
    c = _u8([[1, 1, 0, 0, 2, 2, 0],
             [0, 1, 0, 0, 0, 2, 0],
             [0, 0, 1, 0, 0, 0, 0],
             [2, 0, 0, 0, 1, 1, 1],
             [2, 2, 0, 0, 1, 0, 1]])
    # 8-neighbourhoods: the 1 at (2, 2) hangs on the first patch through its corner
    want8 = np.array([[1, 1, 0, 0, 5, 5, 0],
                      [0, 1, 0, 0, 0, 5, 0],
                      [0, 0, 1, 0, 0, 0, 0],
                      [22, 0, 0, 0, 26, 26, 26],
                      [22, 22, 0, 0, 26, 0, 26]], np.int32)
    want4 = want8.copy()
    want4[2, 2] = 2 * 7 + 2 + 1
    got8, got4 = label_patches_host(c, 3, 8), label_patches_host(c, 3, 4)
    assert got8.dtype == np.int32 and got8.shape == (5, 7)
    assert np.array_equal(got8, want8) and np.array_equal(got4, want4)
    assert np.array_equal(label_patches_host(c, 3), want8)                      # 8 is the default


def test_a_diagonal_pair_is_one_patch_at_8_and_two_at_4():
    c = _u8([[0, 1], [1, 0]])
    assert np.array_equal(label_patches_host(c, 2, 8), [[0, 2], [2, 0]])
    assert np.array_equal(label_patches_host(c, 2, 4), [[0, 2], [3, 0]])


def test_touching_patches_of_classes_1_and_2_stay_apart():
    c = _u8([[1, 2, 2], [1, 1, 2], [0, 2, 1]])
    assert np.array_equal(label_patches_host(c, 3, 8), [[1, 2, 2], [1, 1, 2], [0, 2, 1]])
    assert np.array_equal(label_patches_host(c, 3, 4), [[1, 2, 2], [1, 1, 2], [0, 8, 9]])
    table = measure_patches_host(label_patches_host(c, 3, 8), c)
    assert table.n == 2 and table.cls.tolist() == [1, 2] and table.area.tolist() == [4, 4]
    table = measure_patches_host(label_patches_host(c, 3, 4), c)
    assert table.n == 4 and table.cls.tolist() == [1, 2, 2, 1] and table.area.tolist() == [3, 3, 1, 1]


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("K", [2, 3])
def test_labels_against_a_flood_fill_on_random_maps(K, connectivity):
    rng = np.random.default_rng(100 * K + connectivity)
    for h, w in ((1, 1), (1, 9), (8, 1), (5, 7), (13, 16), (24, 31)):
        for fill in (0.05, 0.45, 0.6, 0.9):
            c = np.where(rng.random((h, w)) < fill, rng.integers(1, K, (h, w)), 0).astype(np.uint8)
            assert np.array_equal(label_patches_host(c, K, connectivity), _flood(c, K, connectivity)), (h, w, fill)


# ---------------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize("connectivity", [4, 8])
def test_measure_against_a_per_patch_nonzero(connectivity):
    rng = np.random.default_rng(connectivity)
    c = np.where(rng.random((24, 31)) < 0.5, rng.integers(1, 3, (24, 31)), 0).astype(np.uint8)
    labels = label_patches_host(c, 3, connectivity)
    t = measure_patches_host(labels, c)
    assert int(t.area.sum()) == np.count_nonzero(c)
    assert t.n == len(np.unique(labels)) - 1 and np.all(np.diff(t.root) > 0)
    assert t.root.dtype == np.int64 and t.cls.dtype == np.uint8 and t.area.dtype == np.int64
    assert t.bbox.dtype == np.int32 and t.bbox.shape == (t.n, 4) and t.sum_y.dtype == np.int64 and t.sum_x.dtype == np.int64
    for r in range(t.n):
        y, x = np.nonzero(labels == t.root[r] + 1)
        assert t.area[r] == len(y) and t.cls[r] == c.ravel()[t.root[r]]
        assert t.bbox[r].tolist() == [y.min(), x.min(), y.max(), x.max()]
        assert t.sum_y[r] == y.sum() and t.sum_x[r] == x.sum()
        assert t.root[r] == (y * 31 + x).min()
    assert np.allclose(t.centroids(), np.stack([t.sum_y / t.area, t.sum_x / t.area], 1), rtol=0, atol=0)
    for a in (t.root, t.cls, t.area, t.bbox, t.sum_y, t.sum_x):
        assert not a.flags.writeable


def test_an_empty_map_has_an_empty_table():
    c = np.zeros((4, 6), np.uint8)
    t = measure_patches_host(label_patches_host(c, 3), c)
    assert t.n == 0 and len(t) == 0 and t.count() == 0 and t.count(1) == 0
    assert t.centroids().shape == (0, 2) and t.area_m2().shape == (0,) and t.bbox.shape == (0, 4)
    assert t.size_histogram([2, 4]).tolist() == [[0, 0, 0]]
    assert t == measure_patches_host(np.zeros((4, 6), np.int32), c)


def test_patch_table_helpers():
    c = _u8([[1, 1, 0, 2, 0, 1],
             [1, 1, 0, 2, 0, 0],
             [0, 0, 0, 2, 0, 2]])
    t = measure_patches_host(label_patches_host(c, 3, 4), c)
    assert t.root.tolist() == [0, 3, 5, 17] and t.cls.tolist() == [1, 2, 1, 2] and t.area.tolist() == [4, 3, 1, 1]
    assert t.n == 4 and t.count() == 4 and t.count(1) == 2 and t.count(2) == 2 and t.count(3) == 0
    assert t.shape == (3, 6)
    assert t.centroids().tolist() == [[0.5, 0.5], [1.0, 3.0], [0.0, 5.0], [2.0, 5.0]]
    assert np.array_equal(t.area_m2(), t.area * PIXEL_AREA_M2) and t.area_m2(2.0).tolist() == [8.0, 6.0, 2.0, 2.0]
    # edges [2, 4]: bins area < 2, 2 <= area < 4, area >= 4; rows class 1, class 2
    assert t.size_histogram([2, 4]).tolist() == [[1, 0, 1], [1, 1, 0]]
    assert t.size_histogram([2, 4], K=4).tolist() == [[1, 0, 1], [1, 1, 0], [0, 0, 0]]
    assert t.size_histogram([1]).tolist() == [[0, 2], [0, 2]]
    for bad in ([], [4, 2], [2, 2]):
        with pytest.raises(ValueError):
            t.size_histogram(bad)
    with pytest.raises(ValueError):
        t.size_histogram([2], K=2)
    same = measure_patches_host(label_patches_host(c, 3, 4), c)
    assert t == same and not (t != same)
    assert t != measure_patches_host(*reversed(sieve_host(c, label_patches_host(c, 3, 4), 2)))
    assert t != "a table" and "n=4" in repr(t)
    with pytest.raises(ValueError):
        t.area[0] = 7
    with pytest.raises(ValueError):
        PatchTable([3, 1], [1, 1], [1, 1], np.zeros((2, 4)), [0, 0], [0, 0], (2, 2))         # roots not ascending
    with pytest.raises(ValueError):
        PatchTable([1, 3], [1], [1, 1], np.zeros((2, 4)), [0, 0], [0, 0], (2, 2))            # ragged columns


# ---------------------------------------------------------------------------------------------- the sieve
@pytest.mark.parametrize("connectivity", [4, 8])
def test_sieve(connectivity):
    rng = np.random.default_rng(40 + connectivity)
    c = np.where(rng.random((24, 31)) < 0.45, rng.integers(1, 3, (24, 31)), 0).astype(np.uint8)
    labels = label_patches_host(c, 3, connectivity)
    full = measure_patches_host(labels, c)
    assert full.area.min() == 1 and full.area.max() >= 6
    for m in (0, 1):                                                             # the identity, as new arrays
        c2, l2 = sieve_host(c, labels, m)
        assert np.array_equal(c2, c) and np.array_equal(l2, labels) and c2 is not c and l2 is not labels
    for m in (2, 5, 24 * 31):
        c2, l2 = sieve_host(c, labels, m)
        keep = np.isin(labels, full.root[full.area >= m] + 1)
        assert np.array_equal(c2, np.where(keep, c, 0)) and np.array_equal(l2, np.where(keep, labels, 0))
        assert np.array_equal(l2, label_patches_host(c2, 3, connectivity))       # the survivors keep their labels
        t = measure_patches_host(l2, c2)
        assert (t.area >= m).all() and t.n == np.count_nonzero(full.area >= m)
        counts = zonal_counts_host(c2, None, 3, 1)
        assert counts[0, 1:].sum() == full.area[full.area >= m].sum() and counts.sum() == c.size
        both, table = patches_host(c, 3, PatchConfig(connectivity, m))
        assert np.array_equal(both, c2) and table == t
    assert np.count_nonzero(sieve_host(c, labels, 24 * 31)[0]) == 0


# ---------------------------------------------------------------------------------------------- errors
def test_value_errors():
    c = _u8([[0, 1], [2, 0]])
    labels = label_patches_host(c, 3)
    with pytest.raises(ValueError, match="out of range"):
        label_patches_host(c, 2)
    for K in (1, 9):
        with pytest.raises(ValueError):
            label_patches_host(c, K)
    for conn in (0, 6, "8"):
        with pytest.raises(ValueError):
            label_patches_host(c, 3, conn)
    for bad in (c.astype(np.int64), c.ravel(), np.zeros((0, 3), np.uint8)):
        with pytest.raises(ValueError):
            label_patches_host(bad, 3)
    with pytest.raises(ValueError):
        measure_patches_host(labels.astype(np.int64), c)
    with pytest.raises(ValueError):
        measure_patches_host(labels[:1], c)
    with pytest.raises(ValueError):
        measure_patches_host(np.zeros_like(labels), c)                           # classes without labels
    with pytest.raises(ValueError):
        measure_patches_host(np.array([[0, 1], [3, 0]], np.int32), c)            # label 1 names pixel 0, which is background
    with pytest.raises(ValueError):
        sieve_host(c, labels, -1)
    with pytest.raises(ValueError):
        sieve_host(c, labels.astype(np.int64), 2)
    for kw in (dict(connectivity=6), dict(connectivity=True), dict(min_pixels=-1), dict(min_pixels=1.5)):
        with pytest.raises(ValueError):
            PatchConfig(**kw)
    assert PatchConfig() == PatchConfig(8, 0) and PatchConfig(4, 3) != PatchConfig(8, 3)
    assert not PatchConfig(8, 1).sieves and PatchConfig(8, 2).sieves and "min_pixels=2" in repr(PatchConfig(8, 2))
    assert check_patches(None) is None and check_patches(False) is None and check_patches(True) == PatchConfig()
    cfg = PatchConfig(4, 9)
    assert check_patches(cfg) is cfg
    for bad in (1, "yes", (8, 0)):
        with pytest.raises(ValueError):
            check_patches(bad)


def test_patches_need_stats_in_infer_tile_and_infer_rasters():
    from deadtrees_amd.deployment.tiler import infer_rasters, infer_tile
    raster = np.zeros((4, 8, 8), np.uint8)
    for patches in (True, PatchConfig(4, 2)):
        with pytest.raises(ValueError, match="stats=True"):
            infer_tile(object(), raster, device="cpu", patches=patches)
        with pytest.raises(ValueError, match="stats=True"):
            next(infer_rasters(object(), [raster], device="cpu", patches=patches))
    with pytest.raises(ValueError, match="PatchConfig"):
        infer_tile(object(), raster, device="cpu", stats=True, patches="all")


# ---------------------------------------------------------------------------------------------- RasterStats, Tiler, shim
def test_raster_stats_carry_a_table():
    c = _u8([[1, 1, 0], [0, 0, 2]])
    table = measure_patches_host(label_patches_host(c, 3), c)
    counts = zonal_counts_host(c, None, 3, 1)
    plain, with_table = RasterStats(counts), RasterStats(counts, patches=table)
    assert plain.patches is None and with_table.patches is table
    assert plain == RasterStats(counts) and repr(plain) == f"RasterStats(counts={counts.tolist()}, pixel_area_m2={PIXEL_AREA_M2!r})"
    assert with_table == RasterStats(counts, patches=measure_patches_host(label_patches_host(c, 3), c))
    assert with_table != plain and plain != with_table
    other = _u8([[1, 0, 1], [0, 0, 2]])
    assert with_table != RasterStats(counts, patches=measure_patches_host(label_patches_host(other, 3), other))
    assert "patches=PatchTable(n=2" in repr(with_table)
    total = with_table + with_table
    assert total.patches is None and np.array_equal(total.counts, 2 * counts) and (plain + with_table).patches is None
    with pytest.raises(ValueError):
        RasterStats(counts, patches=[1, 2])


def test_tiler_stats_with_patches_runs_the_host_contract():
    from deadtrees_amd.deployment.tiler import Tiler
    rng = np.random.default_rng(3)
    c = np.where(rng.random((40, 52)) < 0.3, rng.integers(1, 3, (40, 52)), 0).astype(np.uint8)
    t = Tiler(tile_shape=(64, 64), subtile_shape=(32, 32))
    t.load_array(np.zeros((3, 40, 52), np.uint8))
    t._outdata[:40, :52] = c
    assert t.stats().patches is None
    got = t.stats(patches=True)
    assert np.array_equal(t.result, c) and got.patches == measure_patches_host(label_patches_host(c, 3), c)
    assert np.array_equal(got.counts, zonal_counts_host(c, None, 3, 1))
    got = t.stats(patches=PatchConfig(4, 3))
    want_c, want_l = sieve_host(c, label_patches_host(c, 3, 4), 3)
    assert np.array_equal(t.result, want_c) and got.patches == measure_patches_host(want_l, want_c)
    assert np.array_equal(got.counts, zonal_counts_host(want_c, None, 3, 1)) and (got.patches.area >= 3).all()
    with pytest.raises(ValueError):
        t.stats(patches="yes")


def test_the_reference_shim_exports_the_names():
    import deadtrees.deployment.tiler as shim
    import deadtrees_amd.deployment.tiler as tiler
    assert shim.PatchConfig is PatchConfig and shim.PatchTable is PatchTable
    assert tiler.PatchConfig is PatchConfig and tiler.PatchTable is PatchTable
