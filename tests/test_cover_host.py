"""Cover grids on the host (deployment/cover.py): the numpy definition against a scalar restatement of the contract's two
formulas, the identities that make the grids useful (conservation, aligned grids, additivity across a seam), ``GridConfig``
and ``from_world``, the centroid binning of patches, the CSV rows, every ``ValueError``, and ``RasterStats`` unchanged
without the option.  Integers only: every comparison is exact.  Host only."""
import csv

import numpy as np
import pytest

from deadtrees_amd.deployment import cover
from deadtrees_amd.deployment.cover import CoverGrid, GridConfig, cover_grid_host
from deadtrees_amd.deployment.stats import RasterStats, zonal_counts_host

H, W, K, Z = 37, 106, 3, 3
GRID = GridConfig(cell=7.3, origin=(-2.61, -11.27))


def _maps(h=H, w=W, k=K, z=Z, seed=5):
    rng = np.random.default_rng(seed)
    return rng.integers(0, k, (h, w), dtype=np.uint8), rng.integers(0, z, (h, w), dtype=np.uint8)


def _scalar(classes, zones, k, z, yq, xq):
    """the contract, pixel by pixel and cell by cell, in Python integers"""
    h, w = classes.shape
    sums = np.zeros((len(yq) - 1, len(xq) - 1, z, k), dtype=np.int64)
    for g in range(len(yq) - 1):
        for x in range(len(xq) - 1):
            for i in range(h):
                wy = max(0, min(int(yq[g + 1]), 256 * (i + 1)) - max(int(yq[g]), 256 * i))
                if not wy:
                    continue
                for j in range(w):
                    wx = max(0, min(int(xq[x + 1]), 256 * (j + 1)) - max(int(xq[x]), 256 * j))
                    zone = 0 if zones is None else int(zones[i, j])
                    if wx and zone < z and classes[i, j] < k:
                        sums[g, x, zone, classes[i, j]] += wy * wx
    return sums


def test_the_definition_against_the_scalar_restatement():
    c, z = _maps(9, 13)
    for cell, origin in ((2.7, (-1.3, 0.4)), ((1.0, 3.25), (0.5, -2.125)), (40.0, (-7.0, -9.5)), ((4.0, 1.0), (0.0, 0.0))):
        _, yq, _, xq = GridConfig(cell, origin).edges((9, 13))
        sums, err = cover_grid_host(c, z, K, Z, yq, xq)
        assert sums.dtype == np.int64 and sums.shape == (len(yq) - 1, len(xq) - 1, Z, K) and err == 0
        assert np.array_equal(sums, _scalar(c, z, K, Z, yq, xq)), (cell, origin)
        plain, err = cover_grid_host(c, None, K, 1, yq, xq)
        assert np.array_equal(plain, _scalar(c, None, K, 1, yq, xq)) and err == 0
        assert np.array_equal(plain[:, :, 0], sums.sum(axis=2))
    # tables that cover only a part of the raster, and the weight matrices the contract names
    yq, xq = np.array([300, 700, 1500]), np.array([-100, 256, 1000, 1256])
    sums, _ = cover_grid_host(c, z, K, Z, yq, xq)
    assert np.array_equal(sums, _scalar(c, z, K, Z, yq, xq))
    wy, wx = cover.axis_weights(yq, 9), cover.axis_weights(xq, 13)
    for zone in range(Z):
        for cls in range(K):
            plane = ((c == cls) & (z == zone)).astype(np.int64)
            assert np.array_equal(sums[:, :, zone, cls], np.einsum("gi,ij,xj->gx", wy, plane, wx))


def test_conservation_and_the_aligned_grid():
    c, z = _maps()
    iy0, yq, ix0, xq = GRID.edges((H, W))
    sums, err = cover_grid_host(c, z, K, Z, yq, xq)
    assert err == 0 and np.array_equal(sums.sum(axis=(0, 1)), 65536 * zonal_counts_host(c, z, K, Z))
    grid = CoverGrid.of(sums, (iy0, yq, ix0, xq), (H, W))
    assert np.array_equal(grid.area, sums.sum(axis=(2, 3))) and int(grid.area.sum()) == 65536 * H * W
    assert np.allclose(grid.counts().sum(), H * W) and np.allclose(grid.fraction().sum(axis=2)[grid.area > 0], 1.0)
    # whole-pixel cells on the pixel lattice: a reshape-sum
    c, z = _maps(36, 100)
    _, yq, _, xq = GridConfig((4, 10)).edges((36, 100))
    assert np.array_equal(yq, 1024 * np.arange(10)) and np.array_equal(xq, 2560 * np.arange(11))
    sums, _ = cover_grid_host(c, z, K, Z, yq, xq)
    for zone in range(Z):
        for cls in range(K):
            blocks = ((c == cls) & (z == zone)).reshape(9, 4, 10, 10).sum(axis=(1, 3))
            assert np.array_equal(sums[:, :, zone, cls], 65536 * blocks)


def test_a_raster_cut_at_a_column_that_is_no_cell_edge_merges_to_the_grid_of_the_whole():
    c, z = _maps()
    whole = cover.cover_grid(c, K, GRID, z, n_zones=Z)
    left = cover.cover_grid(c[:, :53], K, GRID, z[:, :53], n_zones=Z)
    right = cover.cover_grid(c[:, 53:], K, GridConfig(7.3, (-2.61, -11.27 - 53)), z[:, 53:], n_zones=Z)
    assert 53 * 256 not in set(whole.xq.tolist())
    merged = CoverGrid.merge([left, right])
    assert (merged.iy0, merged.ix0) == (whole.iy0, whole.ix0) and merged.shape == whole.shape
    assert np.array_equal(merged.sums, whole.sums) and np.array_equal(merged.area, whole.area)
    assert np.array_equal(merged.full, whole.full) and merged == whole and merged.xq is None
    assert left.ix0 == whole.ix0 and right.ix0 > left.ix0 and right.ix0 + right.shape[1] == whole.ix0 + whole.shape[1]
    with pytest.raises(ValueError, match="K / Z differ"):
        CoverGrid.merge([left, cover.cover_grid(c, K, GRID)])
    with pytest.raises(ValueError):
        CoverGrid.merge([])


def test_area_has_its_closed_form_and_covered_tells_the_overhang():
    iy0, yq, ix0, xq = GRID.edges((H, W))
    wy, wx = cover.axis_weights(yq, H), cover.axis_weights(xq, W)
    area = cover.cell_area(yq, xq, (H, W))
    assert np.array_equal(area, wy.sum(axis=1)[:, None] * wx.sum(axis=1)[None, :])
    assert (area > 0).all()                                                      # edges() keeps exactly the cells with area
    grid = CoverGrid.of(np.zeros(area.shape + (1, 2), np.int64), (iy0, yq, ix0, xq), (H, W))
    covered = grid.covered()
    assert covered[1:-1, 1:-1].min() == 1.0 and covered[0, 0] < 1.0 and covered[-1, -1] < 1.0
    assert np.array_equal(grid.full, np.diff(yq)[:, None] * np.diff(xq)[None, :])
    # one more cell on either side would have none
    assert yq[0] < 0 <= yq[1] - 1 and yq[-2] < 256 * H <= yq[-1] and xq[0] < 0 < xq[1] and xq[-2] < 256 * W <= xq[-1]


def test_grid_config_edges_indices_and_hash():
    assert GridConfig(7.3) == GridConfig((7.3, 7.3), (0.0, 0.0)) and hash(GridConfig(7.3)) == hash(GridConfig((7.3, 7.3)))
    assert len({GridConfig(5), GridConfig(5.0), GridConfig(6)}) == 2
    with pytest.raises(Exception):
        GridConfig(5).cell = (6.0, 6.0)                                          # frozen
    iy0, yq, ix0, xq = GridConfig((10, 20), (3.5, -45.25), index0=(100, -7)).edges((50, 64))
    assert iy0 == 99 and yq.tolist() == [256 * v for v in (-6.5, 3.5, 13.5, 23.5, 33.5, 43.5, 53.5)]
    assert ix0 == -5 and xq.tolist() == [256 * v for v in (-5.25, 14.75, 34.75, 54.75, 74.75)]
    assert yq.dtype == np.int64
    # every edge is snapped on its own: floor((o + k c) * 256 + 0.5)
    _, yq, _, _ = GRID.edges((H, W))
    assert yq.tolist() == [int(np.floor((-2.61 + k * 7.3) * 256 + 0.5)) for k in range(len(yq))]
    y, x = GridConfig((10, 20), (3.5, -45.25), index0=(100, -7)).centre(99, np.array([-5, -4]))
    assert float(y) == -1.5 and x.tolist() == [4.75, 24.75]


def test_from_world_lattice_indices_north_up_and_abutting_rasters():
    # 0.25 m pixels, north-up; a 10 m lattice through the world origin
    a = (1000.0, 0.25, 0.0, 5000.0, 0.0, -0.25)
    cfg = GridConfig.from_world(a, 10.0)
    assert cfg.cell == (40.0, 40.0) and cfg.origin == (20000.0, -4000.0)
    iy0, yq, ix0, xq = cfg.edges((100, 120))
    # rows ascend southwards: cell row iy covers Y in [-(iy + 1) * 10, -iy * 10]; the raster's top Y = 5000 -> iy = -500
    assert iy0 == -500 and yq.tolist() == [0, 10240, 20480, 30720] and ix0 == 100 and xq.tolist() == [0, 10240, 20480, 30720]
    # the raster to the east, 120 pixels on, and the one to the south, 100 pixels down: the same lattice, the same indices
    east = GridConfig.from_world((1030.0, 0.25, 0.0, 5000.0, 0.0, -0.25), 10.0).edges((100, 120))
    assert east[0] == iy0 and east[2] == 103 and east[1].tolist() == yq.tolist()
    assert (east[3] + 120 * 256).tolist()[0] == xq[-1]                           # the shared edge, in either frame
    south = GridConfig.from_world((1000.0, 0.25, 0.0, 4975.0, 0.0, -0.25), 10.0).edges((100, 120))
    assert south[0] == -498 and south[1][0] + 100 * 256 == yq[-2] and south[2] == ix0
    # a lattice with its own origin and uneven cells; dy > 0 runs the other way
    cfg = GridConfig.from_world(a, (10.0, 5.0), origin_xy=(2.5, 1.0))
    assert cfg.cell == (40.0, 20.0) and cfg.origin == ((1.0 - 5000.0) / -0.25, (2.5 - 1000.0) / 0.25)
    up = GridConfig.from_world((1000.0, 0.25, 0.0, 5000.0, 0.0, 0.25), 10.0)
    assert up.origin == (-20000.0, -4000.0) and up.edges((100, 120))[0] == 500
    with pytest.raises(ValueError, match="rotated"):
        GridConfig.from_world((0.0, 1.0, 0.1, 0.0, 0.0, -1.0), 10.0)
    with pytest.raises(ValueError):
        GridConfig.from_world((0.0, 1.0, 0.0, 0.0, 0.0), 10.0)
    with pytest.raises(ValueError, match="zero pixel size"):
        GridConfig.from_world((0.0, 0.0, 0.0, 0.0, 0.0, -1.0), 10.0)


def test_abutting_rasters_with_world_grids_merge_to_the_grid_of_the_mosaic():
    c, z = _maps(40, 150)
    t = (1000.0, 0.25, 0.0, 5000.0, 0.0, -0.25)
    whole = cover.cover_grid(c, K, GridConfig.from_world(t, 2.75, (0.5, 0.25)), z, n_zones=Z)
    parts = [cover.cover_grid(c[:, a:b], K, GridConfig.from_world((1000.0 + 0.25 * a,) + t[1:], 2.75, (0.5, 0.25)), z[:, a:b],
                              n_zones=Z) for a, b in ((0, 64), (64, 99), (99, 150))]
    assert CoverGrid.merge(parts) == whole and CoverGrid.merge(parts[::-1]) == whole


def test_values_out_of_range_are_excluded_and_flagged():
    c, z = _maps()
    _, yq, _, xq = GRID.edges((H, W))
    want, _ = cover_grid_host(c, z, K, Z, yq, xq)
    for what, flag in (("class", 1), ("zone", 2), ("both", 3)):
        cc, zz = c.copy(), z.copy()
        where = (np.array([0, 5, 36, 20]), np.array([0, 77, 105, 53]))
        if what in ("class", "both"):
            cc[where[0][:3], where[1][:3]] = (K, 255, K)
        if what in ("zone", "both"):
            zz[where[0][2:], where[1][2:]] = Z
        sums, err = cover_grid_host(cc, zz, K, Z, yq, xq)
        assert err == flag
        bad = (cc >= K) | (zz >= Z)
        assert np.array_equal(sums, _scalar(cc, zz, K, Z, yq, xq))
        assert int(sums.sum()) == 65536 * (H * W - int(bad.sum())) and not np.array_equal(sums, want)
        with pytest.raises(ValueError, match="out of range"):
            cover.cover_grid(cc, K, GRID, zz, n_zones=Z)


def _table(rows, shape, crowns=False):
    """a PatchTable of single-row runs: rows of (cls, y, x0, x1)"""
    from deadtrees_amd.deployment.patches import PatchTable
    rows = sorted(rows, key=lambda r: r[1] * shape[1] + r[2])
    root = [y * shape[1] + x0 for _, y, x0, _ in rows]
    area = [x1 - x0 + 1 for _, _, x0, x1 in rows]
    return PatchTable(root, [r[0] for r in rows], area, [(y, x0, y, x1) for _, y, x0, x1 in rows],
                      [y * a for (_, y, _, _), a in zip(rows, area)], [(x0 + x1) * a // 2 for (_, _, x0, x1), a in zip(rows, area)],
                      shape)


def test_patches_are_binned_by_centroid_half_open():
    yq, xq = np.array([0, 2560, 5120]), np.array([0, 1024, 2048, 4096])
    # centres in pixels: a run x0..x1 of row y has the centre ((x0 + x1 + 1) / 2, y + 0.5)
    rows = [(1, 3, 0, 3),        # x centre 2.0 < 4: cell 0
            (1, 4, 2, 5),        # x centre 4.0, exactly on the edge 1024: cell 1 (half-open)
            (2, 9, 6, 9),        # x centre 8.0, exactly on the edge 2048: cell 2; y centre 9.5 < 10: row 0
            (2, 10, 7, 7),       # y centre 10.5: row 1; x centre 7.5: cell 1
            (1, 19, 15, 15)]     # the last pixel of both axes: centre (15.5, 19.5)
    table = _table(rows, (20, 16))
    count, area = cover.bin_patches(table, yq, xq, 3)
    want = np.zeros((2, 3, 3), np.int64)
    want_area = np.zeros_like(want)
    for (g, x, c), a in {(0, 0, 1): 4, (0, 1, 1): 4, (0, 2, 2): 4, (1, 1, 2): 1, (1, 2, 1): 1}.items():
        want[g, x, c], want_area[g, x, c] = 1, a
    assert np.array_equal(count, want) and np.array_equal(area, want_area)
    # the contract's comparison, as written
    a = table.area
    for k, (g, x) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2))):
        assert 2 * a[k] * xq[x] <= 256 * (2 * table.sum_x[k] + a[k]) < 2 * a[k] * xq[x + 1]
        assert 2 * a[k] * yq[g] <= 256 * (2 * table.sum_y[k] + a[k]) < 2 * a[k] * yq[g + 1]
    # a centroid outside every cell is not counted
    count, _ = cover.bin_patches(table, yq, np.array([1024, 2048]), 3)
    assert int(count.sum()) == 2


def test_patch_figures_through_the_host_pipeline_with_and_without_crowns():
    from deadtrees_amd.deployment.crowns import CrownConfig
    from deadtrees_amd.deployment.tiler import Tiler
    rng = np.random.default_rng(3)
    m = np.zeros((64, 96), np.uint8)
    for _ in range(30):
        y, x = int(rng.integers(0, 58)), int(rng.integers(0, 90))
        m[y:y + int(rng.integers(2, 7)), x:x + int(rng.integers(2, 7))] = rng.integers(1, 3)
    t = Tiler(tile_shape=(64, 96), subtile_shape=(32, 32))
    t.load_array(np.zeros((3, 64, 96), np.uint8))
    t._outdata[...] = m
    grid = GridConfig(9.5, (-3.25, 1.5))
    for crowns in (None, CrownConfig.from_radius(1)):
        stats = t.stats(classes=3, patches=True, grid=grid, crowns=crowns)
        g, table = stats.grid, stats.patches
        assert g.patch_count.shape == g.shape + (3,) and table.n > 5
        for cls in range(3):
            assert int(g.patch_count[:, :, cls].sum()) == table.count(cls)
            assert int(g.patch_area[:, :, cls].sum()) == int(table.area[table.cls == cls].sum())
        want, _ = cover_grid_host(m, None, 3, 1, g.yq, g.xq)
        assert np.array_equal(g.sums, want) and np.array_equal(g.sums.sum(axis=(0, 1)), 65536 * stats.counts)
    assert t.stats(classes=3, grid=grid).grid.patch_count is None


def test_rows_and_the_csv_round_trip(tmp_path):
    c, z = _maps(20, 30, 3, 2)
    grid = cover.cover_grid(c, 3, GridConfig((8.0, 12.5), (-1.0, 2.0), index0=(5, 7)), z)
    rows = grid.rows()
    assert len(rows) == grid.shape[0] * grid.shape[1] and list(rows[0])[:3] == ["iy", "ix", "area_px"]
    assert [r["iy"] for r in rows[::grid.shape[1]]] == list(range(grid.iy0, grid.iy0 + grid.shape[0]))
    assert sum(r["area_px"] for r in rows) == 600.0
    assert sum(r["z1_c2"] for r in rows) == float(np.count_nonzero((z == 1) & (c == 2)))
    t = (1000.0, 0.5, 0.0, 5000.0, 0.0, -0.5)
    rows = grid.rows(t)
    first = rows[0]
    assert first["x"] == 1000.0 + 0.5 * (grid.xq[0] + grid.xq[1]) / 512 and first["y"] == 5000.0 - 0.5 * (grid.yq[0] + grid.yq[1]) / 512
    cfg = GridConfig((8.0, 12.5), (-1.0, 2.0), index0=(5, 7))
    assert [(r["x"], r["y"]) for r in grid.rows(t, cfg)] == [(r["x"], r["y"]) for r in rows]          # 8 and 12.5 snap nowhere
    with pytest.raises(ValueError, match="no pixel frame"):
        CoverGrid.merge([grid]).rows(t)
    path = tmp_path / "cover.csv"
    cover.write_cover_csv(path, grid, t)
    with open(path, newline="") as f:
        back = list(csv.DictReader(f))
    assert len(back) == len(rows) and list(back[0]) == list(rows[0])
    for a, b in zip(back, rows):
        assert {k: float(v) for k, v in a.items()} == {k: float(v) for k, v in b.items()}


def test_the_figures_read_off_a_grid():
    from deadtrees_amd.deployment.stats import forest_dead_percent
    c, z = _maps(40, 60, 3, 2, seed=8)
    z[:, :25] = 0                                                                # the left cells have no forest at all
    grid = cover.cover_grid(c, 3, GridConfig(20), z)
    assert grid.shape == (2, 3)
    dead, share, pct = grid.dead_fraction(), grid.fraction(cls=2, zone=1), grid.forest_dead_percent(limit=10)
    weighted = grid.forest_dead_percent(limit=10, label_weighted=False)
    for g in range(2):
        for x in range(3):
            cc, zz = c[20 * g:20 * g + 20, 20 * x:20 * x + 20], z[20 * g:20 * g + 20, 20 * x:20 * x + 20]
            cell = RasterStats(zonal_counts_host(cc, zz, 3, 2))
            assert dead[g, x] == cell.dead_fraction and share[g, x] == np.count_nonzero((cc == 2) & (zz == 1)) / 400
            for table, flag in ((pct, True), (weighted, False)):
                want = forest_dead_percent(cell, 10, 1, flag)
                if want is None:
                    assert x == 0 and all(np.isnan(table[k][g, x]) for k in table)
                else:
                    assert {k: table[k][g, x] for k in table} == want
    assert grid.fraction().shape == (2, 3, 3) and np.array_equal(grid.counts().sum(axis=(2, 3)), np.full((2, 3), 400.0))
    with pytest.raises(ValueError):
        grid.forest_dead_percent(forest_zone=2)


def test_every_value_error():
    c, z = _maps()
    good = np.arange(0, 5000, 500)
    for cell in (0.99, (5.0, 0.5), -3, float("nan"), (1, 2, 3), "7", True):
        with pytest.raises(ValueError):
            GridConfig(cell)
    with pytest.raises(ValueError):
        GridConfig(5, origin=(float("inf"), 0))
    with pytest.raises(ValueError):
        GridConfig(5, index0=(0.5, 0))
    with pytest.raises(ValueError, match="at least one pixel"):
        cover_grid_host(c, z, K, Z, np.array([0, 255, 600]), good)               # a cell below one pixel
    with pytest.raises(ValueError, match="strictly increasing"):
        cover_grid_host(c, z, K, Z, good, np.array([0, 600, 600, 1200]))         # non-monotone
    with pytest.raises(ValueError, match="strictly increasing"):
        cover_grid_host(c, z, K, Z, good[::-1], good)
    for bad in (np.array([0]), np.array([[0, 300]]), np.array([0.0, 300.0]), np.array([0, 2 ** 23 + 1])):
        with pytest.raises(ValueError):
            cover_grid_host(c, z, K, Z, bad, good)
    with pytest.raises(ValueError, match="more than"):                           # the size bound: 2^26 sums
        cover_grid_host(np.zeros((4000, 4000), np.uint8), np.zeros((4000, 4000), np.uint8), 8, 8,
                        256 * np.arange(1026), 256 * np.arange(1026))
    for k, zz, zones in ((1, 1, None), (9, 1, None), (3, 9, z), (3, 0, z), (3, 2, None)):
        with pytest.raises(ValueError):
            cover_grid_host(c, zones, k, zz, good, good)
    with pytest.raises(ValueError):
        cover_grid_host(c, z[:, :-1], K, Z, good, good)
    with pytest.raises(ValueError):
        cover_grid_host(c.astype(np.int32), z, K, Z, good, good)
    with pytest.raises(ValueError):
        cover.cover_grid(c, K, (7.3, 7.3))
    with pytest.raises(ValueError, match="2\\*\\*23|8388608"):
        GridConfig(32768, origin=(10, 0)).edges((H, W))                          # an edge beyond 2^23


def test_the_request_rules_for_grid():
    from deadtrees_amd.deployment.analysis import MapAnalysis
    from deadtrees_amd.deployment.tiler import infer_rasters, infer_tile

    class Model:
        classes = 3
    raster = np.zeros((3, 40, 40), np.uint8)
    with pytest.raises(ValueError, match="infer_tile: grid needs stats=True"):
        infer_tile(Model(), raster, grid=GRID)
    with pytest.raises(ValueError, match="infer_tile: grid must be a GridConfig or None"):
        infer_tile(Model(), raster, stats=True, grid=(7.3, 7.3))
    with pytest.raises(ValueError, match="infer_rasters: grid needs stats=True"):
        next(infer_rasters(Model(), [raster], grid=GRID))
    with pytest.raises(ValueError, match="infer_rasters: grid needs stats=True"):
        next(infer_rasters(Model(), [raster], grid=lambda key: GRID))
    with pytest.raises(ValueError, match="infer_rasters: grid must be a GridConfig or None"):
        next(infer_rasters(Model(), [raster], stats=True, grid={0: 7.3}))
    with pytest.raises(ValueError, match="Tiler.stats: grid must be"):
        MapAnalysis.rules("Tiler.stats", 3, grid=True)
    request = MapAnalysis.of("infer_tile", (40, 40), 3, grid=GRID)
    assert request.grid == GRID and request.grid_edges[1].tolist() == GRID.edges((40, 40))[1].tolist()
    assert MapAnalysis.of("infer_tile", (40, 40), 3).grid_edges is None
    with pytest.raises(ValueError, match="infer_tile: .*more than"):
        MapAnalysis.of("infer_tile", (4000, 4000), 8, zones=np.full((4000, 4000), 7, np.uint8), grid=GridConfig(1.0))


def test_raster_stats_without_a_grid_are_what_they_were():
    counts = np.array([[5, 1, 0], [3, 2, 1]])
    a, b = RasterStats(counts), RasterStats(counts)
    assert a.grid is None and a == b and "grid" not in repr(a)
    assert repr(a) == f"RasterStats(counts={counts.tolist()}, pixel_area_m2={a.pixel_area_m2!r})"
    assert (a + b) == RasterStats(2 * counts) and (a + b).grid is None
    c, z = _maps(20, 30, 3, 2)
    grid = cover.cover_grid(c, 3, GridConfig(8), z)
    with_grid = RasterStats(zonal_counts_host(c, z, 3, 2), grid=grid)
    assert with_grid.grid is grid and "grid=CoverGrid(" in repr(with_grid)
    assert with_grid != RasterStats(zonal_counts_host(c, z, 3, 2)) and with_grid == RasterStats(with_grid.counts, grid=grid)
    assert with_grid != RasterStats(with_grid.counts, grid=cover.cover_grid(c, 3, GridConfig(9), z))
    assert (with_grid + with_grid).grid is None                                  # CoverGrid.merge is the explicit route
    with pytest.raises(ValueError):
        RasterStats(counts, grid=grid.sums)
    with pytest.raises(ValueError):
        RasterStats(np.ones((1, 3), np.int64), grid=grid)


def test_the_host_path_of_infer_tile_carries_the_grid():
    """``on_device=False`` runs the numpy contract on the merged map"""
    import torch
    from deadtrees_amd.deployment.tiler import infer_tile

    class Model:
        classes = 3

        def run_u8(self, u8, device=None):
            return (u8[..., 0] % 3).to(torch.uint8)
    raster = np.random.default_rng(2).integers(0, 256, (3, 70, 90), dtype=np.uint8)
    zones = (raster[1] % 2).astype(np.uint8)
    base = infer_tile(Model(), raster, subtile=32, on_device=False, device="cpu")
    out, stats = infer_tile(Model(), raster, subtile=32, on_device=False, device="cpu", stats=True, zones=zones, grid=GRID)
    assert np.array_equal(out, base) and np.array_equal(out, raster[0] % 3)
    iy0, yq, ix0, xq = GRID.edges((70, 90))
    assert (stats.grid.iy0, stats.grid.ix0) == (iy0, ix0)
    assert np.array_equal(stats.grid.sums, cover_grid_host(out, zones, 3, 2, yq, xq)[0])
    assert np.array_equal(stats.grid.sums.sum(axis=(0, 1)), 65536 * stats.counts)
