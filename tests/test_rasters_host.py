"""Training from ortho rasters, the host side: the numpy contract of the sub-tile cut and census against a straight-line
loop, the reference's frac / status rounding, the two training sets, the band statistics against a two-pass float64
restatement of scripts/computestats.py:111-161, and the validation of dt_raster_cut_u8 and of the data module.  No GPU."""
import ctypes
import json

import numpy as np
import pytest

from deadtrees_amd.data import rasters as R
from deadtrees_amd.deployment.tiler import make_blocks_vectorized


def _raster(rng, h, w, with_maps=True):
    rgbn = rng.integers(0, 256, (4, h, w), dtype=np.uint8)
    mask = (rng.random((h, w)) < 0.05).astype(np.uint8) * 2 if with_maps else None
    lu = rng.integers(0, 6, (h, w)).astype(np.uint8) if with_maps else None
    return rgbn, mask, lu


def _loop(rgbn, mask, lu, S, t):
    """the contract, one sub-tile at a time"""
    h, w = rgbn.shape[1:]
    x = np.zeros((4, S, S), np.uint8)
    x[:, :h, :w] = rgbn
    m = np.zeros((1, S, S), np.uint8)
    if mask is not None:
        m[0, :h, :w] = mask
    if lu is None:
        l = np.ones((1, S, S), np.uint8)
    else:
        l = np.zeros((1, S, S), np.uint8)
        l[0, :h, :w] = lu
    bx, bm, bl = make_blocks_vectorized(x, t), make_blocks_vectorized(m, t), make_blocks_vectorized(l, t)
    n = (S // t) ** 2
    images, masks, lus = np.zeros((n, t, t, 4), np.uint8), np.zeros((n, t, t), np.uint8), np.zeros((n, t, t), np.uint8)
    sums, census = np.zeros(n, np.uint64), np.zeros((n, 16), np.int64)
    for i in range(n):
        images[i] = np.rollaxis(bx[i], 0, 3)
        masks[i], lus[i] = bm[i, 0], bl[i, 0]
        wide = bx[i].astype(np.int64)
        sums[i] = wide.sum()
        census[i, :6] = [np.count_nonzero(bm[i]), bx[i].min(), bx[i].max(), bx[i][0].min(), bx[i][0].max(),
                         np.count_nonzero((bx[i] != 0) & (bx[i] != 255))]
        census[i, 6:10] = wide.sum(axis=(1, 2))
        census[i, 10:14] = (wide ** 2).sum(axis=(1, 2))
    return images, masks, lus, sums, census


@pytest.mark.parametrize("h,w", [(100, 70), (128, 128)])
@pytest.mark.parametrize("with_maps", [True, False])
def test_cut_raster_host_equals_the_straight_line_loop(h, w, with_maps):
    rng = np.random.default_rng(3)
    rgbn, mask, lu = _raster(rng, h, w, with_maps)
    rgbn[:, 32:64, 0:32] = 77                       # one blank sub-tile
    rgbn[:, 0:32, 32:64] = rng.choice(np.array([0, 255], np.uint8), (4, 32, 32))        # mid == 0
    got = R.cut_raster_host(rgbn, mask, lu, 128, 32)
    want = _loop(rgbn, mask, lu, 128, 32)
    for g, e in zip(got, want):
        assert g.dtype == e.dtype and g.shape == e.shape
        np.testing.assert_array_equal(g, e)
    if not with_maps:
        assert (got[2] == 1).all() and not got[1].any()          # lu: ones in the padded area as well
    elif (h, w) != (128, 128):
        assert not got[2][15].any()                              # a wholly padded sub-tile of a given lu is zeros
    assert got[4][4, 1] == got[4][4, 2] == 77 and got[4][1, 5] == 0


def test_cut_raster_host_rejects_bad_geometry():
    rgbn = np.zeros((4, 40, 40), np.uint8)
    for S, t in ((96, 48), (100, 32), (32, 32)):
        with pytest.raises(ValueError):
            R.cut_raster_host(rgbn, None, None, S, t)
    with pytest.raises(ValueError):
        R.cut_raster_host(rgbn, np.zeros((40, 41), np.uint8), None, 64, 32)


def test_subtile_table_rounding_names_and_blank_rows(tmp_path):
    """at t = 256 three dead pixels are 0.0 % (status 0) and four are 0.01 % (status 1); blank sub-tiles give no row"""
    rng = np.random.default_rng(0)
    rgbn = rng.integers(0, 256, (4, 512, 512), dtype=np.uint8)
    rgbn[:, 256:, 256:] = 9                         # sub-tile 3 is blank
    mask = np.zeros((512, 512), np.uint8)
    mask[0, 0], mask[255, 255], mask[100, 7] = 1, 2, 1                       # three in sub-tile 0
    mask[0, 256], mask[255, 511], mask[10, 300], mask[11, 300] = 1, 1, 3, 1   # four in sub-tile 1
    mask[300, 300] = 1                              # in the blank one
    census = R.cut_raster_host(rgbn, mask, None, 512, 256)[4]
    assert census[:, 0].tolist() == [3, 4, 0, 1]
    rows = R.subtile_table("ortho_7", census, 256)
    assert rows == [("ortho_7_000", 0.0, 0), ("ortho_7_001", 0.01, 1), ("ortho_7_002", 0.0, 0)]
    assert R.subtile_names("a", 12)[-1] == "a_011"
    R.write_subtile_csv(rows, tmp_path / "s.csv")
    assert (tmp_path / "s.csv").read_text().splitlines() == ["tile,frac,status", "ortho_7_000,0.0,0", "ortho_7_001,0.01,1",
                                                            "ortho_7_002,0.0,0"]


def _items(seed=1, n=4, S=128):
    """rasters with a few dead sub-tiles each, one blank sub-tile each, one ragged raster"""
    rng = np.random.default_rng(seed)
    out = []
    for r in range(n):
        h, w = (100, 70) if r == 1 else (S, S)
        rgbn = rng.integers(0, 256, (4, h, w), dtype=np.uint8)
        rgbn[:, 32:64, 32:64] = 200 + r
        mask = np.zeros((h, w), np.uint8)
        for y, x in ((3, 5), (40, 40), (64 + r, 3), (20, 64)):         # (40, 40) lies in the blank sub-tile
            mask[y:y + 4, x:x + 4] = 1
        lu = rng.integers(0, 3, (h, w)).astype(np.uint8)
        out.append((f"ortho_{r}", rgbn, mask, lu if r % 2 else None))
    return out


def test_raster_training_sets_on_host_pools():
    items = _items()
    sets = R.raster_training_sets(items, oversample=2, seed=42, tile_size=32, source_dim=128, device="cpu")
    dead, rnd, table = sets["dead"], sets["random"], sets["table"]
    assert not dead.on_device and dead.shards == [] and dead.height == dead.width == 32
    want = [name for name, frac, status in table if status == 1]
    assert [s["file"] for s in dead.stats] == want and len(dead) == len(want) > 0
    frac = {name: f for name, f, _ in table}
    assert all(s["frac"] == frac[s["file"]] > 0 for s in dead.stats)
    # every dead sample is the host cut of its sub-tile
    cuts = {key: R.cut_raster_host(rgbn, mask, lu, 128, 32) for key, rgbn, mask, lu in items}
    for j, s in enumerate(dead.stats):
        key, i = s["file"].rsplit("_", 1)
        images, masks, lu, sums, _ = cuts[key]
        np.testing.assert_array_equal(dead.images[j], images[int(i)])
        np.testing.assert_array_equal(dead.masks[j], masks[int(i)])
        np.testing.assert_array_equal(dead.lu[j], lu[int(i)])
        assert dead.sums[j] == sums[int(i)] and dead.masks[j].any()
    names = [s["file"] for s in rnd.stats]
    blank = {f"{key}_{i:03}" for key in cuts for i in np.flatnonzero(~R.nonblank(cuts[key][4]))}
    assert 0 < len(rnd) <= 2 * len(dead) and len(set(names)) == len(names)
    assert not set(names) & set(want) and not set(names) & blank
    assert not rnd.masks.any() and all(s["frac"] == 0.0 for s in rnd.stats)
    for j, s in enumerate(rnd.stats):
        key, i = s["file"].rsplit("_", 1)
        np.testing.assert_array_equal(rnd.images[j], cuts[key][0][int(i)])
        np.testing.assert_array_equal(rnd.lu[j], cuts[key][2][int(i)])
    again = R.raster_training_sets(items, oversample=2, seed=42, tile_size=32, source_dim=128, device="cpu")["random"]
    other = R.raster_training_sets(items, oversample=2, seed=43, tile_size=32, source_dim=128, device="cpu")["random"]
    assert [s["file"] for s in again.stats] == names and np.array_equal(again.images, rnd.images)
    assert [s["file"] for s in other.stats] != names
    with pytest.raises(ValueError):
        R.raster_training_sets(iter(items), tile_size=32, source_dim=128, device="cpu")


def test_from_rasters_select_and_resident_bound():
    from deadtrees_amd.data.pool import DevicePool
    items = _items(n=2)
    valid = DevicePool.from_rasters(items, 32, 128, select="valid", device="cpu")
    census = [R.cut_raster_host(rgbn, mask, lu, 128, 32)[4] for _, rgbn, mask, lu in items]
    assert len(valid) == sum(int(R.nonblank(c).sum()) for c in census) and valid.nbytes == len(valid) * (32 * 32 * 6 + 8)
    even = DevicePool.from_rasters(items, 32, 128, select=lambda names, c: np.arange(len(names)) % 2 == 0, device="cpu")
    assert all(int(s["file"][-3:]) % 2 == 0 for s in even.stats) and 0 < len(even) < len(valid)
    with pytest.raises(ValueError, match="max_resident_bytes"):
        DevicePool.from_rasters(items, 32, 128, select="valid", device="cpu", max_resident_bytes=5 * (32 * 32 * 6 + 8))
    with pytest.raises(ValueError):
        DevicePool.from_rasters(items, 32, 128, select="some", device="cpu")
    with pytest.raises(ValueError):
        DevicePool.from_rasters(items, 32, 128, masks="none", device="cpu")


# ------------------------------------------------------------------------------------------------ band statistics
def _two_pass(rasters, t, plus_one=True):
    """computestats.py:111-161 restated in float64: two passes over the rasters as ToTensor hands them over"""
    size = t * t
    mean, std = np.zeros(4), np.zeros(4)
    for stage in (0, 1):
        cnt = 0
        for data in rasters:
            data = data.astype(np.float64) / 255.0
            if data.shape[-2] != data.shape[-1]:
                continue
            if np.isin(data, [0, 1]).all():
                continue
            for sub in make_blocks_vectorized(data, t):
                if sub[0].min() != sub[0].max():
                    if stage == 0:
                        mean += sub.sum((1, 2)) / size
                    else:
                        std += ((sub - mean[:, None, None]) ** 2).sum((1, 2)) / size
                    cnt += 1
        if stage == 0:
            mean /= cnt + 1 if plus_one else cnt
    std = np.sqrt(std / (cnt + 1 if plus_one else cnt))
    return mean, std, cnt


def _stat_rasters(rng):
    """two 320 x 320 rasters of 25 sub-tiles of 64 each; the last row of sub-tiles of each is constant in band 0, so
    2 x 20 = 40 sub-tiles count; per-band standard deviation >= 0.05"""
    out = []
    for r in range(2):
        base = rng.integers(20, 236, (4, 320, 320))
        data = np.clip(base + rng.normal(0, 30, (4, 320, 320)), 0, 255).astype(np.uint8)
        data[0, 256:, :] = 128 + r                 # the last row of sub-tiles: band 0 constant, other bands alive
        out.append(data)
    return out


def test_band_stats_matches_the_two_pass_restatement():
    rng = np.random.default_rng(11)
    rasters = _stat_rasters(rng)
    mean, std, cnt = _two_pass(rasters, 64)
    assert cnt == 40 and std.min() >= 0.05
    items = [(f"r{i}", x, None, None) for i, x in enumerate(rasters)]
    got = R.band_stats(items, source_dim=320, tile_size=64)
    assert got["subtiles"] == 40
    np.testing.assert_allclose(got["mean"], mean, rtol=1e-9, atol=0)
    np.testing.assert_allclose(got["std"], std, rtol=1e-9, atol=0)
    # the same from census tables, bare or with their raster's shape
    census = [R.cut_raster_host(x, None, None, 320, 64)[4] for x in rasters]
    assert R.band_stats(census, 320, 64) == got == R.band_stats([(c, (320, 320)) for c in census], 320, 64)


def test_band_stats_denominator_and_the_three_skips(tmp_path):
    rng = np.random.default_rng(12)
    rasters = _stat_rasters(rng)
    # cnt + 1 against cnt
    m1, s1, cnt = _two_pass(rasters, 64, plus_one=False)
    plain = R.band_stats([(f"r{i}", x, None, None) for i, x in enumerate(rasters)], 320, 64, reference_denominator=False)
    np.testing.assert_allclose(plain["mean"], m1, rtol=1e-9)
    np.testing.assert_allclose(plain["std"], s1, rtol=1e-9)
    ref = R.band_stats([(f"r{i}", x, None, None) for i, x in enumerate(rasters)], 320, 64)
    np.testing.assert_allclose(np.array(ref["mean"]) * (cnt + 1), np.array(plain["mean"]) * cnt, rtol=1e-12)
    # a raster of 0 / 255 only and a raster that is not S x S change nothing; both would otherwise count sub-tiles
    binary = rng.choice(np.array([0, 255], np.uint8), (4, 320, 320))
    ragged = rng.integers(0, 256, (4, 320, 256), dtype=np.uint8)
    more = rasters + [binary, ragged]
    mean, std, cnt2 = _two_pass(more, 64)
    assert cnt2 == cnt == 40
    got = R.band_stats([(f"r{i}", x, None, None) for i, x in enumerate(more)], 320, 64)
    assert got == ref
    np.testing.assert_allclose(got["std"], std, rtol=1e-9)
    assert R.band_stats([R.cut_raster_host(binary, None, None, 320, 64)[4]] + [(f"r{i}", x, None, None) for i, x in
                                                                                enumerate(rasters)], 320, 64) == ref
    # the band-0 filter: the ten sub-tiles with a constant band 0 are alive in the other bands, and not counted
    census = R.cut_raster_host(rasters[0], None, None, 320, 64)[4]
    assert int(R.nonblank(census).sum()) == 25 and int((census[:, 3] != census[:, 4]).sum()) == 20
    info = R.write_band_stats_json(tmp_path / "stats.json", got, sources=["a"])
    back = json.loads((tmp_path / "stats.json").read_text())
    assert back["subtiles"] == 40 and list(back["results"]) == ["red", "green", "blue", "nir"]
    assert back["results"]["nir"] == {"mean": got["mean"][3], "std": got["std"][3]} and info["results"] == back["results"]


# ------------------------------------------------------------------------------------------------ validation
def test_raster_cut_host_side_validation_without_gpu():
    """dt_raster_cut_u8 rejects bad geometry on the host, before any launch, through dt_last_error"""
    from deadtrees_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf)

    def call(h, w, S, t, slot=None, census=p, rgbn=p):
        return lib.dt_raster_cut_u8(rgbn, None, None, h, w, S, t, slot, 0, None, None, None, None, census, None)

    for args, word in (((96, 96, 96, 48), b"multiple of 32"), ((100, 100, 100, 32), b"source_dim"),
                       ((129, 100, 128, 32), b"height and width"), ((100, 0, 128, 32), b"height and width")):
        assert call(*args) != 0
        assert word in lib.dt_last_error(), (args, lib.dt_last_error())
    assert call(100, 70, 128, 32, slot=None, census=None) != 0 and b"both null" in lib.dt_last_error()
    assert call(100, 70, 128, 32, rgbn=None) != 0 and b"null rgbn" in lib.dt_last_error()
    assert call(100, 70, 128, 32, slot=p) != 0 and b"output pointer" in lib.dt_last_error()


def test_data_module_raster_errors():
    from deadtrees_amd.data.deadtreedata import DeadtreesDataModule
    items = _items(n=2)
    with pytest.raises(ValueError, match="alternative"):
        DeadtreesDataModule(rasters=items, pattern="train-*.tar")
    with pytest.raises(ValueError, match="alternative"):
        DeadtreesDataModule(rasters=items, pattern_extra=["x-*.tar"], batch_size_extra=[2])
    with pytest.raises(ValueError, match="more than one"):
        DeadtreesDataModule(rasters=items, batch_size_extra=[2, 2])
    with pytest.raises(ValueError, match="iterator"):
        DeadtreesDataModule(rasters=iter(items))
    with pytest.raises(ValueError, match="normalise"):
        DeadtreesDataModule(rasters=items, normalise="shards")
    dm = DeadtreesDataModule(rasters=items[:1], raster_conf={"tile_size": 32, "source_dim": 128}, device="cpu")
    with pytest.raises(ValueError, match="too few"):          # split_shards's own: one raster, three parts
        dm.setup()


def test_data_module_splits_by_raster_on_host_pools():
    """five rasters -> (3, 1, 1) by sorted key; the pools hold whole rasters; the random set is the one extra pool; the
    constants come from the train part"""
    from deadtrees_amd.data.deadtreedata import DeadtreesDataModule
    items = _items(n=5)
    dm = DeadtreesDataModule(rasters=list(reversed(items)), raster_conf={"tile_size": 32, "source_dim": 128},
                             batch_size_extra=[2], normalise="rasters", device="cpu")
    dm.setup(split_fractions=[0.6, 0.2, 0.2])
    assert dm.shard_split == {"train": ["ortho_0", "ortho_1", "ortho_2"], "val": ["ortho_3"], "test": ["ortho_4"]}
    for name, keys in dm.shard_split.items():
        assert {s["file"].rsplit("_", 1)[0] for s in dm.pools[name].stats} == set(keys)
    assert len(dm.extra_pools) == 1 and set(dm.extra_pools[0]) == {"train", "val"}
    assert not dm.extra_pools[0]["train"].masks.any()
    want = R.band_stats(items[:3], 128, 32)         # (ortho_1 is ragged: skipped)
    assert dm.mean == tuple(want["mean"]) and dm.std == tuple(want["std"]) and want["subtiles"] > 0
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dm.train_dataloader()
