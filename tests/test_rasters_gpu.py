"""Training from ortho rasters on the MI355X: the sub-tile cut and census kernel against the numpy contract
(``cut_raster_host``; integers, so ``array_equal``), a pool filled from rasters against the pool of a shard written from
the same sub-tiles, the batches of both, and the data module's normalisation constants."""
import numpy as np
import pytest
import torch

from shard_fixtures import write_shard

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = 0xA5


def _ragged():
    """S = 128, t = 32, h = 100, w = 70: 16 sub-tiles, column 3 wholly padded, column 2 and row 3 partly"""
    rng = np.random.default_rng(21)
    h, w = 100, 70
    rgbn = rng.integers(0, 256, (4, h, w), dtype=np.uint8)
    rgbn[:, 32:64, 32:64] = 77                      # sub-tile 5: constant, non-zero: blank
    rgbn[:3, 32:64, 0:32] = 50                      # sub-tile 4 varies in band 3 only: vmin != vmax, b0min == b0max
    mask = np.zeros((h, w), np.uint8)
    mask[0, 0], mask[31, 31] = 1, 2                 # first and last pixel of sub-tile 0
    mask[10, 31], mask[10, 32] = 1, 1               # both sides of the border between sub-tiles 0 and 1
    mask[31, 5], mask[32, 5] = 3, 1                 # both sides of the border between sub-tiles 0 and 4
    mask[99, 69] = 1                                # the raster's last pixel
    lu = rng.integers(0, 6, (h, w)).astype(np.uint8)
    slot = rng.permutation(16).astype(np.int32)
    slot[[2, 5, 11]] = -1
    return rgbn, mask, lu, slot


@pytest.fixture(scope="module")
def ragged():
    from deadtrees_amd.data.rasters import cut_raster_host
    rgbn, mask, lu, slot = _ragged()
    return {"in": (rgbn, mask, lu, slot), "full": cut_raster_host(rgbn, mask, lu, 128, 32),
            "bare": cut_raster_host(rgbn, None, None, 128, 32)}


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _pool(rows, t):
    return (torch.full((rows, t, t, 4), FILL, dtype=torch.uint8, device=DEV),
            torch.full((rows, t, t), FILL, dtype=torch.uint8, device=DEV),
            torch.full((rows, t, t), FILL, dtype=torch.uint8, device=DEV),
            torch.full((rows,), -7, dtype=torch.int64, device=DEV))


def _check_pool(out, slot, want):
    """rows that a slot names hold that sub-tile of ``want``; all others still hold the fill"""
    images, masks, lu, sums = (x.cpu().numpy() for x in out)
    named = set()
    for i, r in enumerate(slot.tolist()):
        if r < 0:
            continue
        named.add(r)
        np.testing.assert_array_equal(images[r], want[0][i])
        np.testing.assert_array_equal(masks[r], want[1][i])
        np.testing.assert_array_equal(lu[r], want[2][i])
        assert int(sums[r]) == int(want[3][i])
    for r in set(range(len(sums))) - named:
        assert (images[r] == FILL).all() and (masks[r] == FILL).all() and (lu[r] == FILL).all() and int(sums[r]) == -7
    return len(named)


def test_ragged_raster_matches_the_host_contract(ragged):
    from deadtrees_amd import _lib, ops
    rgbn, mask, lu, slot = ragged["in"]
    want = ragged["full"]
    c = want[4]
    assert c[5, _lib.CENSUS_VMIN] == c[5, _lib.CENSUS_VMAX] == 77                      # the fixture holds what it claims
    assert c[4, _lib.CENSUS_VMIN] != c[4, _lib.CENSUS_VMAX] and c[4, _lib.CENSUS_B0MIN] == c[4, _lib.CENSUS_B0MAX] == 50
    assert c[[3, 7, 11, 15], _lib.CENSUS_VMAX].max() == 0 and c[:, _lib.CENSUS_DEAD].tolist()[:5] == [4, 1, 0, 0, 1]
    out = _pool(16, 32)
    census = ops.raster_cut(_dev(rgbn), _dev(mask), _dev(lu), 128, 32, slot=_dev(slot), out=out)
    np.testing.assert_array_equal(census.cpu().numpy(), c)
    assert _check_pool(out, slot, want) == 13


def test_ragged_raster_variants(ragged):
    from deadtrees_amd import ops
    rgbn, mask, lu, slot = ragged["in"]
    # without mask and land-use map: zeros, and ones in the padded area as well
    out = _pool(16, 32)
    census = ops.raster_cut(_dev(rgbn), None, None, 128, 32, slot=_dev(slot), out=out)
    np.testing.assert_array_equal(census.cpu().numpy(), ragged["bare"][4])
    _check_pool(out, slot, ragged["bare"])
    assert (out[2][int(slot[15])] == 1).all()
    # census only
    only = ops.raster_cut(_dev(rgbn), _dev(mask), _dev(lu), 128, 32)
    np.testing.assert_array_equal(only.cpu().numpy(), ragged["full"][4])
    # cut only
    out = _pool(16, 32)
    assert ops.raster_cut(_dev(rgbn), _dev(mask), _dev(lu), 128, 32, slot=_dev(slot), out=out, census=False) is None
    _check_pool(out, slot, ragged["full"])
    # the wrapper's own checks: both missing, a slot without a pool, a mask of another shape
    with pytest.raises(RuntimeError, match="both null"):
        ops.raster_cut(_dev(rgbn), None, None, 128, 32, census=False)
    with pytest.raises(RuntimeError):
        ops.raster_cut(_dev(rgbn), None, None, 128, 32, slot=_dev(slot))
    with pytest.raises(RuntimeError):
        ops.raster_cut(_dev(rgbn), _dev(mask[:, :-1]), None, 128, 32)


def test_source_one_byte_into_its_allocation(ragged):
    from deadtrees_amd import ops
    rgbn, mask, lu, slot = ragged["in"]
    views = []
    for x in (rgbn, mask, lu):
        buf = torch.empty(x.size + 1, dtype=torch.uint8, device=DEV)
        buf[1:].copy_(_dev(x).reshape(-1))
        views.append(buf[1:].view(x.shape))
        assert views[-1].data_ptr() % 4 == 1 and views[-1].is_contiguous()
    out = _pool(16, 32)
    census = ops.raster_cut(*views, 128, 32, slot=_dev(slot), out=out)
    np.testing.assert_array_equal(census.cpu().numpy(), ragged["full"][4])
    _check_pool(out, slot, ragged["full"])


def test_overflow_and_rounding_case():
    """S = 512, t = 256: a band of all 255 (sumsq = 65536 * 65025 = 4 261 478 400: past 2^31, and 0.8 % short of 2^32
    because 255^2 < 2^16), three against four dead pixels, a sub-tile of 0 and 255 only; then the same raster as ONE
    sub-tile of t = 512 with that band all 255, whose sumsq (262144 * 65025) is past 2^32"""
    from deadtrees_amd import _lib, ops
    from deadtrees_amd.data.rasters import cut_raster_host, subtile_table
    rng = np.random.default_rng(22)
    rgbn = rng.integers(0, 256, (4, 512, 512), dtype=np.uint8)
    rgbn[1, :256, :256] = 255
    rgbn[:, 256:, 256:] = rng.choice(np.array([0, 255], np.uint8), (4, 256, 256))
    mask = np.zeros((512, 512), np.uint8)
    mask[0, 256], mask[255, 511], mask[7, 300] = 1, 1, 2                      # three in sub-tile 1
    mask[256, 0], mask[511, 255], mask[300, 7], mask[300, 8] = 1, 1, 2, 1      # four in sub-tile 2
    want = cut_raster_host(rgbn, mask, None, 512, 256)
    c = want[4]
    assert c[0, _lib.CENSUS_SUMSQ + 1] == 65536 * 65025 > 2 ** 31 and c[3, _lib.CENSUS_MID] == 0
    assert [r[1:] for r in subtile_table("x", c, 256)] == [(0.0, 0), (0.0, 0), (0.01, 1), (0.0, 0)]
    slot = np.array([3, 1, 0, 2], np.int32)
    out = _pool(4, 256)
    census = ops.raster_cut(_dev(rgbn), _dev(mask), None, 512, 256, slot=_dev(slot), out=out)
    np.testing.assert_array_equal(census.cpu().numpy(), c)
    assert _check_pool(out, slot, want) == 4
    rgbn[1] = 255
    want = cut_raster_host(rgbn, mask, None, 512, 512)
    assert want[4][0, _lib.CENSUS_SUMSQ + 1] == 512 * 512 * 65025 > 2 ** 32
    out = _pool(2, 512)
    census = ops.raster_cut(_dev(rgbn), _dev(mask), None, 512, 512, slot=_dev(np.array([1], np.int32)), out=out)
    np.testing.assert_array_equal(census.cpu().numpy(), want[4])
    assert _check_pool(out, np.array([1]), want) == 1


# ------------------------------------------------------------------------------------------------ pools and loaders
S, T = 64, 32


def _small_rasters(n, seed=23):
    """S = 64, t = 32: four sub-tiles each; every raster has dead pixels in sub-tiles 0 and 3 (where it reaches them) and
    a blank sub-tile 1; raster 1 is ragged"""
    rng = np.random.default_rng(seed)
    items = []
    for r in range(n):
        h, w = (50, 64) if r == 1 else (S, S)
        rgbn = rng.integers(0, 256, (4, h, w), dtype=np.uint8)
        rgbn[:, 0:32, 32:64] = 10 + r
        mask = np.zeros((h, w), np.uint8)
        mask[2:6, 3:9] = 1
        mask[40:45, 40:50] = 2
        lu = rng.integers(0, 6, (h, w)).astype(np.uint8)
        items.append((f"ortho_{r}", rgbn, mask, lu if r != 2 else None))
    return items


@pytest.fixture(scope="module")
def two_pools(tmp_path_factory):
    """(the pool from two rasters, the pool from a shard written from the host cut of the same rasters)"""
    from deadtrees_amd.data.pool import DevicePool
    from deadtrees_amd.data.rasters import cut_raster_host, subtile_table
    items = _small_rasters(3)
    samples = []
    for key, rgbn, mask, lu in items:
        images, masks, lus, _, census = cut_raster_host(rgbn, mask, lu, S, T)
        for name, frac, _ in subtile_table(key, census, T):
            i = int(name[-3:])
            samples.append((name, images[i], masks[i], lus[i], frac))
    path = write_shard(tmp_path_factory.mktemp("rasters") / "valid.tar", samples)
    return DevicePool.from_rasters(items, T, S, select="valid", device=DEV), DevicePool([path], device=DEV)


def test_same_pool_from_rasters_as_from_a_shard(two_pools):
    a, b = two_pools
    assert len(a) == len(b) == 9 and a.on_device and a.shards == []
    for name in ("images", "masks", "lu", "sums"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and x.shape == y.shape and x.is_contiguous() and torch.equal(x, y), name
    assert a.stats == b.stats
    assert (a.n, a.height, a.width, a.device, a.nbytes) == (b.n, b.height, b.width, b.device, b.nbytes)


def test_same_batches_from_either_pool(two_pools):
    from deadtrees_amd.data.pool import PoolLoader
    loaders = [PoolLoader(p, 4, train=True, in_channels=4, classes=3, seed=3) for p in two_pools]
    epochs = [list(l) for l in loaders]
    assert len(epochs[0]) == len(epochs[1]) == 2
    for x, y in zip(*epochs):
        (img, mask, dist, lu, stats), other = x["main"], y["main"]
        assert torch.equal(img, other[0]) and torch.equal(mask, other[1]) and torch.equal(dist, other[2])
        assert torch.equal(lu, other[3]) and stats == other[4]


def test_normalisation_constants_from_the_train_rasters():
    from deadtrees_amd.data.deadtreedata import DeadtreesDataModule
    from deadtrees_amd.data.rasters import band_stats, cut_raster_host, subtile_table
    from oracle import augment_ref as A
    items = _small_rasters(5)
    conf = {"batch_size": 2}
    dm = DeadtreesDataModule(rasters=items, raster_conf={"tile_size": T, "source_dim": S}, normalise="rasters",
                             train_dataloader_conf=conf, val_dataloader_conf=conf, test_dataloader_conf=conf, device=DEV)
    dm.setup(split_fractions=[0.6, 0.2, 0.2], in_channels=4, classes=3)
    assert dm.shard_split == {"train": ["ortho_0", "ortho_1", "ortho_2"], "val": ["ortho_3"], "test": ["ortho_4"]}
    want = band_stats([(k, x, None, None) for k, x, _, _ in items[:3]], S, T)
    assert want["subtiles"] == 6                  # two full rasters with three live sub-tiles each; the ragged one is skipped
    for loader in (dm.train_dataloader(), dm.val_dataloader(), dm.test_dataloader()):
        assert loader.mean == tuple(want["mean"]) and loader.std == tuple(want["std"])
    # the val part is the dead sub-tiles of ortho_3, in order, unaugmented
    key, rgbn, mask, lu = items[3]
    images, masks, _, _, census = cut_raster_host(rgbn, mask, lu, S, T)
    dead = [int(name[-3:]) for name, _, status in subtile_table(key, census, T) if status == 1]
    assert dead == [0, 3]
    batches = list(dm.val_dataloader())
    assert len(batches) == 1
    img, got_mask, _, _, stats = batches[0]["main"]
    assert [s["file"] for s in stats] == [f"{key}_{i:03}" for i in dead]
    for b, i in enumerate(dead):
        ref = A.train_transform(images[i], 0, 0, 1.0, 0.0, want["mean"], want["std"], 4).transpose(2, 0, 1)
        np.testing.assert_array_equal(img[b].cpu().numpy(), ref)
        np.testing.assert_array_equal(got_mask[b].cpu().numpy(), masks[i].astype(np.int64))
