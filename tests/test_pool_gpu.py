"""Device-resident pool on the MI355X: the fused batch gather against the kernels it replaces (bit for bit) and against
the numpy oracle, its guard against bad plans, the loader's epochs and the in-place feed of a captured training step."""
import numpy as np
import pytest
import torch

from shard_fixtures import random_samples, stack, write_shard

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 9
SHAPES = [(32, 32), (32, 48), (24, 18)]      # square: all 12 views; W % 4 == 0 and W % 4 == 2 (scalar tail): flips, half turns


def _pool(h, w, seed=0):
    """host arrays of a pool of N random samples with labels {0, 1, 2}; sample 1 is bright enough to reach the clip"""
    rng = np.random.default_rng(seed)
    images = rng.integers(0, 256, (N, h, w, 4), dtype=np.uint8)
    images[1] = np.clip(images[1].astype(np.int32) + 150, 0, 255)
    masks = rng.integers(0, 3, (N, h, w)).astype(np.uint8)
    lu = rng.integers(0, 6, (N, h, w)).astype(np.uint8)
    sums = images.reshape(N, -1).astype(np.int64).sum(axis=1)
    return images, masks, lu, sums


def _calls(h, w, seed=1):
    """three batches of 5: repeated indices in non-monotonic order; all 12 flip x turn pairs on square tiles (flips and
    half turns otherwise); parameter rows (1, 0) next to random draws"""
    rng = np.random.default_rng(seed)
    views = [(f, r) for r in (0, 1, 2, 3) for f in (0, 1, 2)] if h == w else [(f, r) for r in (0, 2) for f in (0, 1, 2)]
    views = (views * 3)[:15]
    idx = [[7, 1, 4, 1, 0], [3, 8, 1, 2, 6], [5, 1, 8, 0, 5]]
    out = []
    for k in range(3):
        geo = np.array(views[5 * k:5 * k + 5], np.int32)
        bc = np.array([[1.0, 0.0] if (b + k) % 3 == 0 else [1 + rng.uniform(-.15, .15), rng.uniform(-.2, .2)]
                       for b in range(5)], np.float32)
        out.append((np.array(idx[k], np.int32), geo, bc))
    return out


def _dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)


def _merged(masks_u8, merge):
    m = masks_u8.long()
    return torch.where(m > 1, torch.ones_like(m), m) if merge else m


@pytest.mark.parametrize("merge", [0, 1])
@pytest.mark.parametrize("c_dst", [3, 4])
@pytest.mark.parametrize("h,w", SHAPES)
def test_gather_is_bit_identical_to_the_unfused_kernels(h, w, c_dst, merge):
    """img == augment_normalize_u8(images[idx]) in NCHW, labels == augment_labels of the (merged) .long() maps"""
    from deadtrees_amd import ops
    from deadtrees_amd.data.synthetic import MEAN, STD
    images, masks, lu, sums = _dev(*_pool(h, w))
    seen = set()
    for idx, geo, bc in _calls(h, w):
        seen |= {tuple(g) for g in geo.tolist()}
        idx, geo, bc = _dev(idx, geo, bc)
        img, mask, lu_out, err = ops.pool_gather_batch(images, masks, lu, sums, idx, geo, bc, MEAN, STD, c_dst, merge)
        assert img.dtype == torch.float32 and tuple(img.shape) == (5, c_dst, h, w) and img.is_contiguous()
        assert mask.dtype == torch.int64 and lu_out.dtype == torch.int64
        sel = idx.long()
        want = ops.augment_normalize_u8(images[sel], geo, bc, MEAN, STD, c_dst).permute(0, 3, 1, 2)
        assert torch.equal(img, want)
        assert torch.equal(mask, ops.augment_labels(_merged(masks[sel], merge), geo))
        assert torch.equal(lu_out, ops.augment_labels(lu[sel].long(), geo))          # lu is never merged
        assert int(err) == 0
        assert int(mask.max()) == (1 if merge else 2)
    assert len(seen) == (12 if h == w else 6)
    # without a land-use map, into given buffers
    idx, geo, bc = _dev(*_calls(h, w)[0])
    out = (torch.full((5, c_dst, h, w), 7.0, device=DEV), torch.full((5, h, w), 7, dtype=torch.int64, device=DEV), None)
    img2, mask2, none, _ = ops.pool_gather_batch(images, masks, None, sums, idx, geo, bc, MEAN, STD, c_dst, merge, out=out)
    assert img2 is out[0] and mask2 is out[1] and none is None
    first = ops.pool_gather_batch(images, masks, lu, sums, idx, geo, bc, MEAN, STD, c_dst, merge)
    assert torch.equal(img2, first[0]) and torch.equal(mask2, first[1])


@pytest.mark.parametrize("h,w", SHAPES)
def test_gather_matches_the_numpy_oracle(h, w):
    """oracle/augment_ref.py on images[idx]: exact where the parameters are (1, 0); elsewhere the cap
    tests/test_surface_gpu.py grants this arithmetic (<= 1 grey level, < 1 % of entries off by more than 1e-3 grey level
    — a margin: tests/test_shards_host.py shows the fp32 formula itself is bit-equal to the oracle)."""
    from deadtrees_amd import ops
    from deadtrees_amd.data.synthetic import MEAN, STD
    from oracle import augment_ref as A
    host = _pool(h, w)
    images, masks, lu, sums = _dev(*host)
    grey = (np.asarray(STD[:4], np.float32) * 255.0)[:, None, None]
    for idx, geo, bc in _calls(h, w):
        img, mask, lu_out, _ = ops.pool_gather_batch(images, masks, lu, sums, *_dev(idx, geo, bc), MEAN, STD, 4, 1)
        img, mask, lu_out = img.cpu().numpy(), mask.cpu().numpy(), lu_out.cpu().numpy()
        for b in range(5):
            s, (f, r), (al, be) = int(idx[b]), geo[b].tolist(), bc[b].tolist()
            want = A.train_transform(host[0][s], f, r, al, be, MEAN, STD, 4).transpose(2, 0, 1)
            if al == 1.0 and be == 0.0:
                np.testing.assert_array_equal(img[b], want)
            else:
                diff = np.abs(img[b] - want) * grey
                assert float(diff.max()) <= 1.0 + 1e-3 and float((diff > 1e-3).mean()) < 1e-2
            np.testing.assert_array_equal(mask[b], A.geometric(np.minimum(host[1][s], 1).astype(np.int64), f, r))
            np.testing.assert_array_equal(lu_out[b], A.geometric(host[2][s].astype(np.int64), f, r))


def test_gather_guard_zeroes_bad_samples_and_flags_them():
    """an index of N or -1 (and an odd turn of a non-square tile) never reaches the pool: zeros, a bit of the flag, and
    the other samples of the batch as usual"""
    from deadtrees_amd import ops
    from deadtrees_amd.data.synthetic import MEAN, STD
    images, masks, lu, sums = _dev(*_pool(32, 48))
    idx = torch.tensor([2, N, 0, -1, 5], dtype=torch.int32, device=DEV)
    geo = torch.tensor([[1, 2], [0, 0], [2, 0], [1, 0], [0, 2]], dtype=torch.int32, device=DEV)
    bc = torch.tensor([[1.1, 0.1], [1.0, 0.0], [0.9, -0.1], [1.1, 0.1], [1.0, 0.0]], device=DEV)
    img, mask, lu_out, err = ops.pool_gather_batch(images, masks, lu, sums, idx, geo, bc, MEAN, STD, 3, 0)
    assert int(err) == 1
    good = torch.tensor([0, 2, 4], device=DEV)
    sel = idx.long()[good]
    for bad in (1, 3):
        assert not img[bad].any() and not mask[bad].any() and not lu_out[bad].any()
    assert torch.equal(img[good], ops.augment_normalize_u8(images[sel], geo[good], bc[good], MEAN, STD, 3).permute(0, 3, 1, 2))
    assert torch.equal(mask[good], ops.augment_labels(masks[sel].long(), geo[good]))
    assert torch.equal(lu_out[good], ops.augment_labels(lu[sel].long(), geo[good]))
    geo[2, 1] = 1
    img, mask, _, err = ops.pool_gather_batch(images, masks, lu, sums, idx[:3], geo[:3], bc[:3], MEAN, STD, 3, 0)
    assert int(err) == 3 and not img[2].any() and not mask[2].any() and bool(img[0].any())


def test_gather_offsets_past_4_gib():
    """a pool of 2^20 + 4 tiles of 32x32 holds 4 GiB of image bytes: samples past 2^31 and past 2^32 bytes come back
    right (all offsets are 64-bit).  The pool is zeros but for the samples read."""
    from deadtrees_amd import ops
    from deadtrees_amd.data.synthetic import MEAN, STD
    n, h, w = (1 << 20) + 4, 32, 32
    images = torch.zeros((n, h, w, 4), dtype=torch.uint8, device=DEV)
    masks = torch.zeros((n, h, w), dtype=torch.uint8, device=DEV)
    sums = torch.zeros(n, dtype=torch.int64, device=DEV)
    where = torch.tensor([(1 << 19) + 1, n - 1, 3], device=DEV)
    small = _dev(*_pool(h, w, seed=5))
    images[where], masks[where], sums[where] = small[0][:3], small[1][:3], small[3][:3]
    idx = torch.tensor([n - 1, 3, (1 << 19) + 1, (1 << 19) + 2], dtype=torch.int32, device=DEV)
    geo = torch.tensor([[1, 1], [0, 0], [2, 3], [0, 0]], dtype=torch.int32, device=DEV)
    bc = torch.tensor([[1.1, 0.15], [1.0, 0.0], [0.9, -0.1], [1.0, 0.0]], device=DEV)
    img, mask, _, err = ops.pool_gather_batch(images, masks, None, sums, idx, geo, bc, MEAN, STD, 4, 0)
    sel = idx.long()
    assert torch.equal(img, ops.augment_normalize_u8(images[sel], geo, bc, MEAN, STD, 4).permute(0, 3, 1, 2))
    assert torch.equal(mask, ops.augment_labels(masks[sel].long(), geo))
    assert int(err) == 0 and bool(mask[:3].any()) and not mask[3].any()
    del images, masks
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ loader and trainer binding
SEED = 5


@pytest.fixture(scope="module")
def shard_dir(tmp_path_factory):
    """five shards -> split (3, 1, 1): train 3 x 6 samples, val 10, test 5, all 32x32"""
    d = tmp_path_factory.mktemp("shards")
    rng = np.random.default_rng(9)
    parts = []
    for i, n in enumerate((6, 6, 6, 10, 5)):
        samples = random_samples(rng, n, 32, 32, f"s{i}")
        write_shard(d / f"shard_{i}.tar", samples, compression="tiff_lzw" if i == 1 else None)
        parts.append(samples)
    return str(d), {"train": stack(parts[0] + parts[1] + parts[2]), "val": stack(parts[3]), "test": stack(parts[4])}


def _datamodule(shard_dir, **kw):
    from deadtrees_amd.data.deadtreedata import DeadtreesDataModule
    conf = {"batch_size": 4}
    dm = DeadtreesDataModule(shard_dir[0], "shard_*.tar", train_dataloader_conf=conf, val_dataloader_conf=conf,
                             test_dataloader_conf=conf, device=DEV, seed=SEED, **kw)
    dm.setup(in_channels=3, classes=2)
    return dm


def _check_batch(item, host, idx, geo, bc, classes=2):
    """one yielded tuple against the numpy oracle applied to its rows of the plan"""
    from deadtrees_amd.data.distmap import distmaps_on_device
    from deadtrees_amd.data.synthetic import MEAN, STD
    from oracle import augment_ref as A
    images, masks, lu, keys, fracs = host
    img, mask, dist, lu_out, stats = item
    assert img.dtype == torch.float32 and tuple(img.shape) == (4, 3, 32, 32) and img.is_contiguous() and img.is_cuda
    assert mask.dtype == torch.int64 and lu_out.dtype == torch.int64 and tuple(mask.shape) == tuple(lu_out.shape) == (4, 32, 32)
    assert dist.dtype == torch.float32 and tuple(dist.shape) == (4, classes, 32, 32)
    assert torch.equal(dist, distmaps_on_device(mask, classes))
    assert stats == [{"file": keys[i], "frac": fracs[i]} for i in idx.tolist()]
    grey = (np.asarray(STD[:3], np.float32) * 255.0)[:, None, None]
    got, gm, gl = img.cpu().numpy(), mask.cpu().numpy(), lu_out.cpu().numpy()
    for b, s in enumerate(idx.tolist()):
        (f, r), (al, be) = geo[b].tolist(), bc[b].tolist()
        want = A.train_transform(images[s], f, r, al, be, MEAN, STD, 3).transpose(2, 0, 1)
        if al == 1.0 and be == 0.0:
            np.testing.assert_array_equal(got[b], want)
        else:
            diff = np.abs(got[b] - want) * grey
            assert float(diff.max()) <= 1.0 + 1e-3 and float((diff > 1e-3).mean()) < 1e-2
        np.testing.assert_array_equal(gm[b], A.geometric(np.minimum(masks[s], 1).astype(np.int64), f, r))
        np.testing.assert_array_equal(gl[b], A.geometric(lu[s].astype(np.int64), f, r))


def test_loader_epochs_follow_the_plan(shard_dir):
    from deadtrees_amd.data.pool import epoch_plan
    dm = _datamodule(shard_dir)
    assert {k: len(p) for k, p in dm.pools.items()} == {"train": 18, "val": 10, "test": 5}
    pool = dm.pools["train"]
    assert pool.on_device and pool.images.dtype == torch.uint8 and tuple(pool.images.shape) == (18, 32, 32, 4)
    np.testing.assert_array_equal(pool.images.cpu().numpy(), shard_dir[1]["train"][0])
    np.testing.assert_array_equal(pool.sums.cpu().numpy(),
                                  shard_dir[1]["train"][0].reshape(18, -1).astype(np.int64).sum(axis=1))
    loader = dm.train_dataloader()
    assert len(loader) == 4
    epochs = []
    for epoch in range(2):                       # plain iteration: epoch 0, then epoch 1
        batches = [b["main"] for b in loader]
        assert loader.epoch == epoch and len(batches) == len(loader)
        idx, geo, bc = epoch_plan(18, 4, epoch, SEED, True, True)
        for k, item in enumerate(batches):
            _check_batch(item, shard_dir[1]["train"], idx[4 * k:4 * k + 4], geo[4 * k:4 * k + 4], bc[4 * k:4 * k + 4])
        epochs.append(batches)
    assert not all(torch.equal(a[0], b[0]) for a, b in zip(*epochs))        # reshuffled, redrawn
    loader.set_epoch(0)
    again = [b["main"] for b in loader]
    assert loader.epoch == 0
    for a, b in zip(epochs[0], again):
        assert all(torch.equal(a[i], b[i]) for i in range(4)) and a[4] == b[4]


def test_val_and_test_loaders_are_sequential_and_unaugmented(shard_dir):
    dm = _datamodule(shard_dir)
    neutral = (torch.zeros((4, 2), dtype=torch.int32), torch.tensor([[1.0, 0.0]] * 4))
    val = dm.val_dataloader()
    assert len(val) == 2                          # 10 samples: the partial batch is dropped
    for _ in range(2):                            # every epoch alike
        batches = list(val)
        assert len(batches) == 2 and all(set(b) == {"main"} for b in batches)
        for k, b in enumerate(batches):
            _check_batch(b["main"], shard_dir[1]["val"], torch.arange(4 * k, 4 * k + 4), *neutral)
    test = list(dm.test_dataloader())
    assert len(test) == 1 and isinstance(test[0], tuple)          # the bare tuple of the reference's test loader
    _check_batch(test[0], shard_dir[1]["test"], torch.arange(4), *neutral)


def test_loader_feeds_the_captured_step_in_place(shard_dir):
    """fit() on a graph trainer bound to the loader: once the step is captured, the loader yields the very tensors
    ``static_batch()`` names (filled by the gather), so the step's staging copies do not run"""
    from deadtrees_amd.network.unet import UNetHIP
    from deadtrees_amd.trainer import HipTrainer, fit
    dm = _datamodule(shard_dir)
    tr = HipTrainer(UNetHIP().to(DEV), graph=True, losses=("GDICE", "FOCAL", "BOUNDARY-RAMPED"))
    loader = dm.train_dataloader(trainer=tr)
    seen = []

    class Recorder:
        def __iter__(self):
            for batch in loader:
                img, mask, dist = batch["main"][:3]
                seen.append((img, mask, dist, tr.static_batch()))
                yield batch

    val = dm.val_dataloader()
    history = fit(tr, Recorder(), epochs=2, val_loader=val)
    assert len(seen) == 8 and [h["epoch"] for h in history] == [0, 1]
    assert all(np.isfinite(h["train/total_loss"]) and np.isfinite(h["val/total_loss"]) for h in history)
    assert all(h["val/samples"] == len(val) * 4 == 8 for h in history)
    for k, (img, mask, dist, static) in enumerate(seen):
        assert dist is None                       # the captured step computes the distance maps itself
        if k % 4 == 3:                            # two eager steps, capture on the third, the fourth is fed in place
            assert static is not None and img is static[0] and mask is static[1] and static[2] is None
        if k in (1, 2, 5, 6):                     # no graph yet (BOUNDARY-RAMPED re-captures every epoch): fresh tensors
            assert static is None
    last = tr.static_batch()
    assert seen[-1][0] is last[0] and seen[-1][1] is last[1]
    # what the captured step last read is the last batch of epoch 1's plan
    want = [b["main"] for b in _replay(dm, 1)][-1]
    assert torch.equal(last[0], want[0]) and torch.equal(last[1], want[1])


def _replay(dm, epoch):
    loader = dm.train_dataloader()
    loader.set_epoch(epoch)
    return list(loader)
