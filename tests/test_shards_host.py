"""Webdataset shards on the host: reader and grouping, the reference's split rules, the epoch plan, and what a machine
without a HIP device can and cannot do with a shard directory."""
import numpy as np
import pytest
import torch

from shard_fixtures import random_samples, stack, write_shard


# ------------------------------------------------------------------ reader and grouping
def test_read_shard_round_trip(tmp_path):
    """2 shards x 5 samples of 32x32, one LZW-compressed: arrays, keys, frac and the byte sums come back exactly"""
    from deadtrees_amd.data.shards import read_shard, shard_len
    rng = np.random.default_rng(0)
    for name, comp in (("a.tar", None), ("b.tar", "tiff_lzw")):
        samples = random_samples(rng, 5, 32, 32, name[0])
        path = write_shard(tmp_path / name, samples, compression=comp)
        got = read_shard(path)
        images, masks, lu, keys, fracs = stack(samples)
        assert got["images"].dtype == np.uint8 and got["images"].shape == (5, 32, 32, 4)
        np.testing.assert_array_equal(got["images"], images)
        np.testing.assert_array_equal(got["masks"], masks)
        np.testing.assert_array_equal(got["lu"], lu)
        assert got["keys"] == keys
        assert got["stats"] == [{"file": k, "frac": f} for k, f in zip(keys, fracs)]
        assert got["sums"].dtype == np.uint64
        np.testing.assert_array_equal(got["sums"], images.reshape(5, -1).astype(np.uint64).sum(axis=1))
        assert shard_len(path) == 5


def test_three_band_image_gets_opaque_fourth_band(tmp_path):
    from deadtrees_amd.data.shards import read_shard
    samples = random_samples(np.random.default_rng(1), 2, 32, 32, "rgb", bands=3)
    got = read_shard(write_shard(tmp_path / "rgb.tar", samples))
    np.testing.assert_array_equal(got["images"][..., :3], np.stack([s[1] for s in samples]))
    assert (got["images"][..., 3] == 255).all()


def test_bad_samples_raise_value_error_naming_shard_and_key(tmp_path):
    from deadtrees_amd.data.shards import read_shard
    rng = np.random.default_rng(2)
    ok = random_samples(rng, 3, 32, 32, "ok")
    p = write_shard(tmp_path / "nolu.tar", ok, skip={("ok_001", "lu.tif")})
    with pytest.raises(ValueError, match=r"nolu\.tar.*ok_001.*lu\.tif"):
        read_shard(p)
    p = write_shard(tmp_path / "mixed.tar", ok[:2] + random_samples(rng, 1, 32, 64, "wide"))
    with pytest.raises(ValueError, match=r"mixed\.tar.*wide_000"):
        read_shard(p)
    p = write_shard(tmp_path / "odd.tar", random_samples(rng, 2, 48, 40, "odd"))
    with pytest.raises(ValueError, match=r"odd\.tar.*odd_000.*32"):
        read_shard(p)


def test_grouping_follows_the_webdataset_key_rule(tmp_path):
    """the key is the member path up to the first '.' of the basename; directories belong to it"""
    from deadtrees_amd.data.shards import read_shard, split_key
    assert split_key("a/b.rgbn.tif") == ("a/b", "rgbn.tif")
    assert split_key("a.b/c.txt") == ("a.b/c", "txt")
    assert split_key("x.mask.tif") == ("x", "mask.tif")
    assert split_key("README") == (None, None)
    rng = np.random.default_rng(3)
    samples = [(f"d{i}/tile", *s[1:]) for i, s in enumerate(random_samples(rng, 3, 32, 32, "t"))]
    got = read_shard(write_shard(tmp_path / "dirs.tar", samples))
    assert got["keys"] == ["d0/tile", "d1/tile", "d2/tile"]          # same basename, different samples
    np.testing.assert_array_equal(got["masks"], np.stack([s[2] for s in samples]))


# ------------------------------------------------------------------ split rules
THREE_WAY = {4: (2, 1, 1), 5: (3, 1, 1), 8: (6, 1, 1), 10: (7, 2, 1), 15: (10, 3, 2), 25: (18, 5, 2)}
TWO_WAY = {1: (0, 1), 2: (1, 1), 7: (6, 1)}


def _names(n):
    names = [f"shard_{i:03d}.tar" for i in range(n)]
    return names, list(np.random.default_rng(n).permutation(names))


def _assert_contiguous(parts, names):
    at = 0
    for part in parts:
        assert part == names[at:at + len(part)]
        at += len(part)
    assert at == len(names)


@pytest.mark.parametrize("n", sorted(THREE_WAY))
def test_split_shards_three_way_table(n):
    from deadtrees.data.deadtreedata import split_shards          # the shim exports it as the reference does
    names, shuffled = _names(n)
    parts = split_shards(shuffled, [0.7, 0.2, 0.1])
    assert tuple(len(p) for p in parts) == THREE_WAY[n]
    _assert_contiguous(parts, names)


@pytest.mark.parametrize("n", sorted(TWO_WAY))
def test_split_shards_two_way_table(n):
    from deadtrees_amd.data.shards import split_shards
    names, shuffled = _names(n)
    parts = split_shards(shuffled, [0.8, 0.2])
    assert parts[2] is None
    assert tuple(len(p) for p in parts[:2]) == TWO_WAY[n]
    _assert_contiguous(parts[:2], names)


def test_split_shards_exceptions():
    from deadtrees_amd.data.shards import split_shards
    with pytest.raises(ValueError):
        split_shards(_names(3)[1], [0.7, 0.2, 0.1])
    with pytest.raises(AssertionError):
        split_shards(_names(10)[1], [0.7, 0.2, 0.2])


def test_shards_for_rank():
    from deadtrees_amd.data.shards import shards_for_rank
    shards = list("abcdefg")
    assert shards_for_rank(shards, 0, 1) == shards
    assert [shards_for_rank(shards, r, 3) for r in range(3)] == [["a", "d", "g"], ["b", "e"], ["c", "f"]]
    with pytest.raises(ValueError):
        shards_for_rank(shards[:2], 2, 3)
    with pytest.raises(ValueError):
        shards_for_rank(shards, 3, 3)


# ------------------------------------------------------------------ epoch plan
def test_epoch_plan_train():
    from deadtrees_amd.data.pool import epoch_plan
    idx, geo, bc = epoch_plan(18, 4, 0, 7, True, True)
    assert idx.dtype == torch.int32 and geo.dtype == torch.int32 and bc.dtype == torch.float32
    assert tuple(idx.shape) == (16,) and tuple(geo.shape) == (16, 2) and tuple(bc.shape) == (16, 2)    # partial batch dropped
    assert len(set(idx.tolist())) == 16 and 0 <= int(idx.min()) and int(idx.max()) < 18
    full = epoch_plan(18, 3, 0, 7, True, True)[0]
    assert sorted(full.tolist()) == list(range(18))                 # a permutation
    assert full.tolist()[:16] == idx.tolist()                       # the order does not depend on the batch size
    again = epoch_plan(18, 4, 0, 7, True, True)
    assert all(torch.equal(a, b) for a, b in zip((idx, geo, bc), again))
    other = epoch_plan(18, 4, 1, 7, True, True)
    assert not torch.equal(other[0], idx) and not torch.equal(other[2], bc)
    assert not torch.equal(epoch_plan(18, 4, 0, 8, True, True)[0], idx)
    assert set(geo[:, 0].tolist()) <= {0, 1, 2} and set(geo[:, 1].tolist()) <= {0, 1, 2, 3}
    assert float(bc[:, 0].min()) >= 0.85 and float(bc[:, 0].max()) <= 1.15 and float(bc[:, 1].abs().max()) <= 0.2


def test_epoch_plan_eval_is_identity_with_neutral_parameters():
    from deadtrees_amd.data.pool import epoch_plan
    for epoch in (0, 5):
        idx, geo, bc = epoch_plan(11, 4, epoch, 3, False, True)
        assert idx.tolist() == list(range(8)) and idx.dtype == torch.int32
        assert geo.dtype == torch.int32 and not geo.any() and tuple(geo.shape) == (8, 2)
        assert bc.dtype == torch.float32 and torch.equal(bc, torch.tensor([[1.0, 0.0]] * 8))


def test_epoch_plan_draws_no_odd_turn_on_non_square_tiles():
    from deadtrees_amd.data.pool import epoch_plan
    turns = set()
    for epoch in range(4):
        sq = epoch_plan(64, 8, epoch, 1, True, True)
        ns = epoch_plan(64, 8, epoch, 1, True, False)
        turns |= set(ns[1][:, 1].tolist())
        assert torch.equal(sq[0], ns[0]) and torch.equal(sq[2], ns[2]) and torch.equal(sq[1][:, 0], ns[1][:, 0])
    assert turns == {0, 2}
    assert {1, 3} <= set(torch.cat([epoch_plan(64, 8, e, 1, True, True)[1][:, 1] for e in range(4)]).tolist())


# ------------------------------------------------------------------ the kernel's formula
def test_fp32_restatement_of_the_gather_formula_equals_the_oracle():
    """``gather_formula`` — per pixel v*alpha + add, clip, floor, normalise, all in fp32, add = fp32(fp64(beta) * sum /
    (4*H*W)) — is bit-equal to oracle/augment_ref.py (a 256-entry LUT) on 80 random cases of the shapes the GPU tests use:
    the one-grey-level cap those tests grant the device is a margin the arithmetic does not need."""
    from deadtrees_amd.data.synthetic import MEAN, STD
    from oracle import augment_ref as A
    rng = np.random.default_rng(11)
    for case in range(80):
        h, w = [(32, 32), (32, 48), (24, 18)][case % 3]
        img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        if case % 5 == 0:
            img = np.clip(img.astype(np.int32) + 150, 0, 255).astype(np.uint8)
        flip = int(rng.integers(0, 3))
        rot = int(rng.integers(0, 4)) if h == w else 2 * int(rng.integers(0, 2))
        alpha, beta = np.float32(1 + rng.uniform(-.15, .15)), np.float32(rng.uniform(-.2, .2))
        c = 3 + case % 2
        want = A.train_transform(img, flip, rot, float(alpha), float(beta), MEAN, STD, c)
        got = gather_formula(A.geometric(img, flip, rot), int(img.sum(dtype=np.uint64)), alpha, beta, MEAN, STD, c)
        np.testing.assert_array_equal(got, want)


def gather_formula(img_u8_hwc, total, alpha, beta, mean, std, c_dst):
    """the arithmetic of csrc/pool.hip on an already flipped / turned image, in numpy fp32"""
    h, w, _ = img_u8_hwc.shape
    v = img_u8_hwc[..., :c_dst].astype(np.float32)
    if not (alpha == 1 and beta == 0):
        add = np.float32(0) if beta == 0 else np.float32(np.float64(beta) * (np.float64(total) / (float(h) * w * 4)))
        v = np.floor(np.clip(v * np.float32(alpha) + add, np.float32(0), np.float32(255)))
    m = np.asarray(mean[:c_dst], np.float32) * np.float32(255)
    inv = np.float32(1) / (np.asarray(std[:c_dst], np.float32) * np.float32(255))
    return (v - m) * inv


# ------------------------------------------------------------------ without a HIP device
def test_datamodule_setup_on_a_shard_directory_without_gpu(tmp_path):
    """(where there is a HIP device, device="cpu" asks for the same host pools)"""
    from deadtrees_amd.data.deadtreedata import DeadtreesDataModule
    host = {"device": "cpu"} if torch.cuda.is_available() else {}
    rng = np.random.default_rng(4)
    want = []
    for i in range(4):        # [0.7, 0.2, 0.1] of 4 shards -> (2, 1, 1)
        samples = random_samples(rng, 3 + i, 32, 32, f"s{i}")
        write_shard(tmp_path / f"shard_{i}.tar", samples, compression="tiff_adobe_deflate" if i == 1 else None)
        want.append(samples)
    dm = DeadtreesDataModule(str(tmp_path), "shard_*.tar", train_dataloader_conf={"batch_size": 2}, **host)
    dm.setup(in_channels=3, classes=2)
    assert {k: len(p) for k, p in dm.pools.items()} == {"train": 7, "val": 5, "test": 6}
    train = dm.pools["train"]
    assert not train.on_device and (train.height, train.width) == (32, 32)
    images, masks, lu, keys, _ = stack(want[0] + want[1])
    np.testing.assert_array_equal(train.images, images)
    np.testing.assert_array_equal(train.masks, masks)
    np.testing.assert_array_equal(train.lu, lu)
    assert train.sums.dtype == np.uint64
    np.testing.assert_array_equal(train.sums, images.reshape(7, -1).astype(np.uint64).sum(axis=1))
    assert [s["file"] for s in train.stats] == keys
    with pytest.raises(RuntimeError):
        dm.train_dataloader()
    # data parallel: shard i of the train part to rank i % world
    dm1 = DeadtreesDataModule(str(tmp_path), "shard_*.tar", rank=1, world=2, **host)
    dm1.setup()
    assert len(dm1.pools["train"]) == 4 and dm1.pools["train"].stats[0]["file"] == "s1_000"
    with pytest.raises(NotImplementedError):
        DeadtreesDataModule(str(tmp_path), "shard_*.tar", pattern_extra=["extra_*.tar"], batch_size_extra=[2])
    with pytest.raises(ValueError, match="max_resident_bytes"):
        DeadtreesDataModule(str(tmp_path), "shard_*.tar", max_resident_bytes=1000, **host).setup()
