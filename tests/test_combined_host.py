"""Combined shard sets on the host: the data module's constructor rules and the split of the extra sets, the combined
epoch plan (``max_size_cycle`` over loaders batched with ``partial=False``) and the batch type ``create_combined_batch``
passes through.  Nothing here needs a HIP device."""
import numpy as np
import pytest
import torch

from shard_fixtures import random_samples, stack, write_shard

MAIN, NEG, RND = (6, 6, 6, 10, 5), (3, 3, 3, 3), (2, 2, 2, 2)
EXTRA = {"pattern_extra": ["neg_*.tar", "rnd_*.tar"], "batch_size_extra": [1, 2]}


def write_sets(d, seed=9):
    """main_0..4 (6, 6, 6, 10, 5 samples), neg_0..3 (3 each), rnd_0..3 (2 each), all 32x32 -> {name: [samples per shard]}"""
    rng = np.random.default_rng(seed)
    parts = {}
    for name, counts in (("main", MAIN), ("neg", NEG), ("rnd", RND)):
        parts[name] = []
        for i, n in enumerate(counts):
            samples = random_samples(rng, n, 32, 32, f"{name}{i}")
            write_shard(d / f"{name}_{i}.tar", samples)
            parts[name].append(samples)
    return parts


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    d = tmp_path_factory.mktemp("combined")
    return d, write_sets(d)


def _dm(d, **kw):
    from deadtrees_amd.data.deadtreedata import DeadtreesDataModule
    conf = {"batch_size": 6}
    kw = {**EXTRA, "train_dataloader_conf": conf, "val_dataloader_conf": conf, "test_dataloader_conf": {"batch_size": 4},
          "device": "cpu", **kw}
    return DeadtreesDataModule(str(d), "main_*.tar", **kw)


# ------------------------------------------------------------------ constructor
def test_constructor_errors(sets, tmp_path):
    from deadtrees_amd.data.deadtreedata import DeadtreesDataModule
    d = str(sets[0])
    with pytest.raises(ValueError, match="train/val/test layout not allowed"):
        DeadtreesDataModule([d, d, d], "main_*.tar", **EXTRA)
    with pytest.raises(ValueError, match="don't match"):
        DeadtreesDataModule(d, "main_*.tar", pattern_extra=["neg_*.tar", "rnd_*.tar"], batch_size_extra=[2])
    with pytest.raises(ValueError, match="batch_size_extra"):
        DeadtreesDataModule(d, "main_*.tar", pattern_extra=["neg_*.tar"])
    with pytest.raises(ValueError, match="pattern_extra"):
        DeadtreesDataModule(d, "main_*.tar", batch_size_extra=[2])
    with pytest.raises(NotImplementedError):          # the synthetic source: no shard matches `pattern`
        DeadtreesDataModule(str(tmp_path), "main_*.tar", **EXTRA)
    with pytest.raises(NotImplementedError):
        DeadtreesDataModule(None, None, **EXTRA)
    with pytest.raises(NotImplementedError):          # an extra pattern without a shard: nothing to cycle
        DeadtreesDataModule(d, "main_*.tar", pattern_extra=["neg_*.tar", "none_*.tar"], batch_size_extra=[1, 2])
    dm = DeadtreesDataModule(d, "main_*.tar", **EXTRA)
    assert [len(s) for s in dm.data_shards_extra] == [4, 4] and dm.batch_size_extra == [1, 2]
    assert DeadtreesDataModule(d, "main_*.tar").data_shards_extra == []


def test_batch_size_must_leave_a_main_sample(sets):
    """batch_size - sum(batch_size_extra) < 1 is a ValueError of the loader that is asked for, train or val"""
    dm = _dm(sets[0], train_dataloader_conf={"batch_size": 3}, val_dataloader_conf={"batch_size": 2})
    dm.setup()
    with pytest.raises(ValueError, match="batch_size 3"):
        dm.train_dataloader()
    with pytest.raises(ValueError, match="batch_size 2"):
        dm.val_dataloader()


# ------------------------------------------------------------------ setup
def test_setup_splits_every_extra_set_like_the_main_one(sets):
    d, parts = sets
    dm = _dm(d)
    dm.setup(in_channels=3, classes=2)
    assert {k: len(p) for k, p in dm.pools.items()} == {"train": 18, "val": 10, "test": 5}      # main split (3, 1, 1)
    assert [{k: len(p) for k, p in e.items()} for e in dm.extra_pools] == [{"train": 9, "val": 3}, {"train": 6, "val": 2}]
    for e, name in zip(dm.extra_pools, ("neg", "rnd")):        # train_frac 0.75: a 4-shard set splits (3, 1)
        images, masks, lu, keys, _ = stack(sum(parts[name][:3], []))
        assert not e["train"].on_device
        np.testing.assert_array_equal(e["train"].images, images)
        np.testing.assert_array_equal(e["train"].masks, masks)
        np.testing.assert_array_equal(e["train"].lu, lu)
        np.testing.assert_array_equal(e["train"].sums, images.reshape(len(keys), -1).astype(np.uint64).sum(axis=1))
        assert [s["file"] for s in e["train"].stats] == keys
        assert [s["file"] for s in e["val"].stats] == stack(parts[name][3])[3]
    for ask in (dm.train_dataloader, dm.val_dataloader, dm.test_dataloader):      # host pools make no batches
        with pytest.raises(RuntimeError):
            ask()


def test_extra_train_shards_follow_the_rank(sets):
    d, parts = sets
    dm = _dm(d, rank=1, world=2)
    dm.setup()
    assert len(dm.pools["train"]) == 6
    assert [len(e["train"]) for e in dm.extra_pools] == [3, 2] and [len(e["val"]) for e in dm.extra_pools] == [3, 2]
    assert [s["file"] for s in dm.extra_pools[0]["train"].stats] == stack(parts["neg"][1])[3]      # shards i % 2 == 1
    assert [s["file"] for s in dm.extra_pools[1]["train"].stats] == stack(parts["rnd"][1])[3]


def test_one_shard_extra_set_and_other_tile_size_raise(tmp_path):
    parts = write_sets(tmp_path)
    rng = np.random.default_rng(1)
    write_shard(tmp_path / "single_0.tar", random_samples(rng, 4, 32, 32, "single"))
    for i in range(4):
        write_shard(tmp_path / f"wide_{i}.tar", random_samples(rng, 2, 32, 64, f"wide{i}"))
    assert len(parts["main"]) == 5
    with pytest.raises(ValueError, match=r"single_\*\.tar"):
        _dm(tmp_path, pattern_extra=["neg_*.tar", "single_*.tar"]).setup()
    with pytest.raises(ValueError, match=r"wide_\*\.tar.*32x64"):
        _dm(tmp_path, pattern_extra=["neg_*.tar", "wide_*.tar"]).setup()


# ------------------------------------------------------------------ plans
def test_epoch_plan_default_stream_is_the_plain_generator():
    from deadtrees_amd.data.deadtreedata import draw_train_params
    from deadtrees_amd.data.pool import epoch_plan
    seed, epoch = 7, 3
    idx, geo, bc = epoch_plan(18, 4, epoch, seed, True, True)
    rng = np.random.default_rng([seed, epoch])
    want = rng.permutation(18)[:16].astype(np.int32)
    g, b = draw_train_params(16, rng)
    assert idx.tolist() == want.tolist() and torch.equal(geo, g) and torch.equal(bc, b)
    assert all(torch.equal(x, y) for x, y in zip(epoch_plan(18, 4, epoch, seed, True, True, stream=()), (idx, geo, bc)))
    rng = np.random.default_rng([seed, epoch, 2, 1])
    other = epoch_plan(18, 4, epoch, seed, True, True, stream=(2, 1))
    assert other[0].tolist() == rng.permutation(18)[:16].tolist() and other[0].tolist() != idx.tolist()


NS, BS = (18, 9, 6), (3, 1, 2)


def _rows(t, k, j):
    """rows of source j in batch k of a plan tensor"""
    lo = 6 * k + sum(BS[:j])
    return t[lo:lo + BS[j]]


def test_combined_plan_cycles_the_shorter_sources():
    from deadtrees_amd.data.pool import combined_plan, epoch_plan
    seed, epoch = 5, 2
    L, src, idx, geo, bc = combined_plan(NS, BS, epoch, seed, True, True)
    assert L == 9                                           # lens 6, 9, 3
    assert src.dtype == idx.dtype == geo.dtype == torch.int32 and bc.dtype == torch.float32
    assert tuple(src.shape) == tuple(idx.shape) == (54,) and tuple(geo.shape) == tuple(bc.shape) == (54, 2)
    assert src.tolist() == [0, 0, 0, 1, 2, 2] * 9           # the row order inside a batch
    for j, n in enumerate(NS):
        assert 0 <= int(idx[src == j].min()) and int(idx[src == j].max()) < n

    def check(j, first, count, stream):
        """batches first .. first+count-1 of source j are the head of epoch_plan(..., stream)"""
        want = epoch_plan(NS[j], BS[j], epoch, seed, True, True, stream=stream)
        for got, ref in zip((idx, geo, bc), want):
            rows = torch.cat([_rows(got, first + p, j) for p in range(count)])
            assert torch.equal(rows, ref[:count * BS[j]])
        return torch.cat([_rows(idx, first + p, j) for p in range(count)]).tolist()

    main = check(0, 0, 6, ())                               # == a plain PoolLoader(pool, 3) epoch
    assert sorted(main) == list(range(18))
    assert idx.reshape(9, 6)[:6, :3].reshape(-1).tolist() == epoch_plan(18, 3, epoch, seed, True, True)[0].tolist()
    again = check(0, 6, 3, (0, 1))                          # the main set starts over: a fresh permutation's head
    assert len(set(again)) == 9
    assert sorted(check(1, 0, 9, (1, 0))) == list(range(9))
    cycles = [check(2, 3 * c, 3, (2, c)) for c in range(3)]     # source 2 runs three cycles without repeats inside one
    assert all(sorted(c) == list(range(6)) for c in cycles) and len({tuple(c) for c in cycles}) > 1
    # deterministic in (seed, epoch)
    same = combined_plan(NS, BS, epoch, seed, True, True)
    assert same[0] == L and all(torch.equal(a, b) for a, b in zip(same[1:], (src, idx, geo, bc)))
    assert not torch.equal(combined_plan(NS, BS, epoch + 1, seed, True, True)[2], idx)
    assert not torch.equal(combined_plan(NS, BS, epoch, seed + 1, True, True)[2], idx)
    # non-square tiles: no odd turn anywhere, everything else as drawn
    ns = combined_plan(NS, BS, epoch, seed, True, False)
    assert set(ns[3][:, 1].tolist()) <= {0, 2} and torch.equal(ns[2], idx) and torch.equal(ns[4], bc)


def test_combined_plan_eval_cycles_are_arange():
    from deadtrees_amd.data.pool import combined_plan
    for epoch in (0, 4):
        L, src, idx, geo, bc = combined_plan(NS, BS, epoch, 5, False, True)
        assert L == 9 and src.tolist() == [0, 0, 0, 1, 2, 2] * 9
        for k in range(9):
            assert _rows(idx, k, 0).tolist() == list(range(3 * (k % 6), 3 * (k % 6) + 3))
            assert _rows(idx, k, 1).tolist() == [k]
            assert _rows(idx, k, 2).tolist() == list(range(2 * (k % 3), 2 * (k % 3) + 2))
        assert not geo.any() and torch.equal(bc, torch.tensor([[1.0, 0.0]] * 54))


def test_combined_plan_errors():
    from deadtrees_amd.data.pool import combined_plan
    with pytest.raises(ValueError, match="source 2"):
        combined_plan((18, 9, 1), BS, 0, 0, True, True)          # len 0: nothing to cycle
    with pytest.raises(ValueError):
        combined_plan((18, 9), BS, 0, 0, True, True)
    with pytest.raises(ValueError):
        combined_plan(NS, (3, 0, 2), 0, 0, True, True)
    L, src, idx, _, _ = combined_plan((7,), (2,), 0, 0, True, True)      # one source: a plain epoch
    assert L == 3 and not src.any() and len(set(idx.tolist())) == 6


@pytest.mark.parametrize("n,b", [(37, 4), (8, 8), (9, 2), (5, 1)])
def test_combined_plan_of_one_source_is_the_epoch_plan(n, b):
    """what lets ``PoolLoader`` and ``CombinedPoolLoader`` be one loader: one source makes ``combined_plan`` the plain
    ``epoch_plan``, value for value and dtype for dtype"""
    from deadtrees_amd.data.pool import combined_plan, epoch_plan
    seed = 11
    for train in (True, False):
        for square in (True, False):
            for epoch in (0, 3):
                L, src, *rows = combined_plan([n], [b], epoch, seed, train, square)
                want = epoch_plan(n, b, epoch, seed, train, square)
                assert L == n // b and src.dtype == torch.int32 and tuple(src.shape) == (L * b,) and not src.any()
                assert len(rows) == len(want) == 3
                for got, ref in zip(rows, want):
                    assert got.dtype == ref.dtype and torch.equal(got, ref)


# ------------------------------------------------------------------ batch type
def test_combined_batch_passes_through_create_combined_batch():
    from deadtrees.network.segmodel import create_combined_batch as shim
    from deadtrees_amd.data.pool import CombinedBatch
    from deadtrees_amd.network.segmodel import create_combined_batch
    g = torch.Generator().manual_seed(0)
    img, dist = torch.randn(6, 3, 4, 4, generator=g), torch.randn(6, 2, 4, 4, generator=g)
    mask, lu = torch.randint(0, 2, (6, 4, 4), generator=g), torch.randint(0, 6, (6, 4, 4), generator=g)
    stats = [{"file": f"f{i}", "frac": i / 6} for i in range(6)]
    batch = CombinedBatch((img, mask, dist, lu, stats), BS)
    assert isinstance(batch, dict) and list(batch) == ["main", "extra_0", "extra_1"]
    assert [v[0].shape[0] for v in batch.values()] == [3, 1, 2] and all(len(v) == 5 for v in batch.values())
    assert batch["extra_1"][0].data_ptr() == img[4:].data_ptr() and batch["extra_0"][4] == stats[3:4]
    for fn in (create_combined_batch, shim):
        out = fn(batch)
        assert all(a is b for a, b in zip(out, (img, mask, dist, lu, stats)))       # the objects themselves
    old = create_combined_batch(dict(batch))                                         # a plain dict: the torch.cat path
    assert old[0] is not img and all(torch.equal(a, b) for a, b in zip(old[:4], (img, mask, dist, lu))) and old[4] == stats
    none = CombinedBatch((img, mask, None, lu, stats), BS)                           # a loader without distance maps
    assert none.combined[2] is None and all(v[2] is None for v in none.values())
    assert create_combined_batch(dict(none))[2] is None
    with pytest.raises(ValueError):
        CombinedBatch((img, mask, dist, lu, stats), (3, 1))
