"""Combined shard sets on the MI355X: ``dt_pool_gather_combined`` against ``dt_pool_gather_batch`` slot by slot (bit for
bit), its guard, 64-bit offsets inside a second source, the combined loader against the numpy oracle and the in-place feed
of a captured training step."""
import numpy as np
import pytest
import torch

from shard_fixtures import random_samples, stack, write_shard

pytestmark = pytest.mark.gpu
DEV = "cuda"
NS = (9, 4, 3)
SRC = [0, 2, 1, 0, 1, 2, 0]
IDX = [7, 2, 3, 1, 0, 1, 8]                     # 7 and 8 exist in source 0 only
SHAPES = [(32, 32), (32, 48), (24, 18)]         # all 12 views; flips and half turns; W % 4 == 2: the scalar tail


def _dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)


def _pool(n, h, w, seed):
    """device arrays of n random samples with labels {0, 1, 2}; sample 1 is bright enough to reach the clip"""
    rng = np.random.default_rng(seed)
    images = rng.integers(0, 256, (n, h, w, 4), dtype=np.uint8)
    images[1] = np.clip(images[1].astype(np.int32) + 150, 0, 255)
    masks = rng.integers(0, 3, (n, h, w)).astype(np.uint8)
    lu = rng.integers(0, 6, (n, h, w)).astype(np.uint8)
    return _dev(images, masks, lu, images.reshape(n, -1).astype(np.int64).sum(axis=1))


_SOURCES = {}


def _sources(h, w):
    """the three pools of one shape, made once and left unchanged"""
    if (h, w) not in _SOURCES:
        _SOURCES[(h, w)] = [_pool(n, h, w, seed=10 + j) for j, n in enumerate(NS)]
    return _SOURCES[(h, w)]


def _calls(h, w):
    """two batches of 7 over all 12 flip x turn pairs (6 on non-square tiles); rows (1, 0) next to random draws; the
    bright sample (slot 3: sample 1 of source 0) gets the strongest draw in the first batch"""
    rng = np.random.default_rng(1)
    views = [(f, r) for r in (0, 1, 2, 3) for f in (0, 1, 2)] if h == w else [(f, r) for r in (0, 2) for f in (0, 1, 2)]
    views = (views * 3)[:14]
    out = []
    for k in range(2):
        geo = np.array(views[7 * k:7 * k + 7], np.int32)
        bc = np.array([[1.0, 0.0] if (b + k) % 3 == 0 else [1 + rng.uniform(-.15, .15), rng.uniform(-.2, .2)]
                       for b in range(7)], np.float32)
        if k == 0:
            bc[3] = (1.15, 0.2)
        out.append(_dev(np.array(SRC, np.int32), np.array(IDX, np.int32), geo, bc))
    return out


def _assert_slots_equal_single_source(got, sources, src, idx, geo, bc, c_dst, merge, with_lu=True):
    """every slot of ``got`` equals ops.pool_gather_batch on its source's arrays with that slot's rows"""
    from deadtrees_amd import ops
    from deadtrees_amd.data.synthetic import MEAN, STD
    for j, (images, masks, lu, sums) in enumerate(sources):
        sel = (src == j).nonzero().flatten()
        if not len(sel):
            continue
        want = ops.pool_gather_batch(images, masks, lu if with_lu else None, sums, idx[sel].contiguous(),
                                     geo[sel].contiguous(), bc[sel].contiguous(), MEAN, STD, c_dst, merge)
        assert int(want[3]) == 0
        assert torch.equal(got[0][sel], want[0]) and torch.equal(got[1][sel], want[1])
        if with_lu:
            assert torch.equal(got[2][sel], want[2])


@pytest.mark.parametrize("merge", [0, 1])
@pytest.mark.parametrize("c_dst", [3, 4])
@pytest.mark.parametrize("h,w", SHAPES)
def test_combined_gather_is_bit_identical_to_the_single_pool_kernel(h, w, c_dst, merge):
    from deadtrees_amd import ops
    from deadtrees_amd.data.synthetic import MEAN, STD
    sources = _sources(h, w)
    seen = set()
    for src, idx, geo, bc in _calls(h, w):
        seen |= {tuple(g) for g in geo.tolist()}
        img, mask, lu, err = ops.pool_gather_combined(sources, src, idx, geo, bc, MEAN, STD, c_dst, merge)
        assert img.dtype == torch.float32 and tuple(img.shape) == (7, c_dst, h, w) and img.is_contiguous()
        assert mask.dtype == lu.dtype == torch.int64 and tuple(mask.shape) == tuple(lu.shape) == (7, h, w)
        assert int(err) == 0 and int(mask.max()) == (1 if merge else 2) and int(lu.max()) > 1
        _assert_slots_equal_single_source((img, mask, lu), sources, src, idx, geo, bc, c_dst, merge)
    assert len(seen) == (12 if h == w else 6)
    # the clip is reached: the brightest draw on the bright sample saturates some pixel of band 0
    src, idx, geo, bc = _calls(h, w)[0]
    img = ops.pool_gather_combined(sources, src, idx, geo, bc, MEAN, STD, c_dst, merge)[0]
    assert float(img[3, 0].max()) == pytest.approx((255.0 - MEAN[0] * 255.0) / (STD[0] * 255.0), rel=1e-6)
    # one source: the whole batch equals dt_pool_gather_batch
    one = sources[0]
    zero = torch.zeros(7, dtype=torch.int32, device=DEV)
    idx0 = torch.tensor([7, 1, 4, 1, 0, 8, 3], dtype=torch.int32, device=DEV)
    got = ops.pool_gather_combined([one], zero, idx0, geo, bc, MEAN, STD, c_dst, merge)
    want = ops.pool_gather_batch(*one, idx0, geo, bc, MEAN, STD, c_dst, merge)
    assert all(torch.equal(a, b) for a, b in zip(got[:3], want[:3])) and int(got[3]) == 0
    # without land-use maps, into given buffers, ORing into a given flag
    bare = [(i, m, None, s) for i, m, _, s in sources]
    out = (torch.full((7, c_dst, h, w), 7.0, device=DEV), torch.full((7, h, w), 7, dtype=torch.int64, device=DEV), None)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    img2, mask2, none, err2 = ops.pool_gather_combined(bare, src, idx, geo, bc, MEAN, STD, c_dst, merge, out=out, err=flag)
    assert img2 is out[0] and mask2 is out[1] and none is None and err2 is flag and int(flag) == 0
    _assert_slots_equal_single_source((img2, mask2, None), sources, src, idx, geo, bc, c_dst, merge, with_lu=False)


@pytest.mark.parametrize("c_dst", [3, 4])
@pytest.mark.parametrize("h,w", SHAPES)
def test_one_source_without_src_is_the_zero_src_and_the_single_pool_call(h, w, c_dst):
    from deadtrees_amd import ops
    from deadtrees_amd.data.synthetic import MEAN, STD
    sources = _sources(h, w)
    one = sources[0]
    src, _, geo, bc = _calls(h, w)[0]
    idx0 = torch.tensor([7, 1, 4, 1, 0, 8, 3], dtype=torch.int32, device=DEV)
    got = ops.pool_gather_combined([one], None, idx0, geo, bc, MEAN, STD, c_dst, 1)
    zero = ops.pool_gather_combined([one], torch.zeros_like(src), idx0, geo, bc, MEAN, STD, c_dst, 1)
    single = ops.pool_gather_batch(*one, idx0, geo, bc, MEAN, STD, c_dst, 1)
    assert tuple(got[0].shape) == (7, c_dst, h, w) and bool(got[0].any()) and int(got[1].max()) == 1
    for other in (zero, single):
        assert all(torch.equal(a, b) for a, b in zip(got[:3], other[:3]))
        assert int(got[3]) == 0 and int(other[3]) == 0
    with pytest.raises(RuntimeError, match="one source"):
        ops.pool_gather_combined(sources[:2], None, idx0, geo, bc, MEAN, STD, c_dst, 1)
    # the C entry dt_pool_gather_batch itself (ops reaches the kernel through dt_pool_gather_combined): its one row
    import ctypes as C
    from deadtrees_amd import _lib
    images, masks, lu, sums = one
    img, mask, lu_out, flag = (torch.full_like(t, 7) for t in got)
    mean, std = ((C.c_float * c_dst)(*v[:c_dst]) for v in (MEAN, STD))

    def entry(lu_in, n):
        p = _lib.ptr
        return _lib.load().dt_pool_gather_batch(p(images), p(masks), p(lu_in), p(sums), p(idx0), p(geo), p(bc), p(img),
                                                p(mask), p(lu_out), p(flag.zero_()), n, 7, h, w, c_dst, 1, mean, std,
                                                _lib.stream())
    _lib.check(entry(lu, images.shape[0]), "dt_pool_gather_batch")
    assert all(torch.equal(a, b) for a, b in zip((img, mask, lu_out), got[:3])) and int(flag) == 0
    _lib.check(entry(lu, 8), "dt_pool_gather_batch")             # N = 8 puts sample 8 (slot 5) outside the pool
    assert int(flag) == 1 and not img[5].any() and torch.equal(img[:5], got[0][:5]) and torch.equal(mask[6], got[1][6])
    with pytest.raises(RuntimeError, match="pool_gather_batch: lu and lu_out go together"):
        _lib.check(entry(None, images.shape[0]), "dt_pool_gather_batch")
    with pytest.raises(RuntimeError, match="pool_gather_batch: "):
        _lib.check(entry(lu, 0), "dt_pool_gather_batch")


def test_combined_gather_checks_its_arguments():
    from deadtrees_amd import ops
    from deadtrees_amd.data.synthetic import MEAN, STD
    sources = _sources(32, 32)
    src, idx, geo, bc = _calls(32, 32)[0]
    with pytest.raises(RuntimeError, match="tiles"):
        ops.pool_gather_combined([sources[0], _sources(32, 48)[1]], src, idx, geo, bc, MEAN, STD, 3)
    with pytest.raises(RuntimeError, match="lu in every source or in none"):
        ops.pool_gather_combined([sources[0], sources[1][:2] + (None,) + sources[1][3:]], src, idx, geo, bc, MEAN, STD, 3)
    with pytest.raises(RuntimeError, match="sources"):
        ops.pool_gather_combined([sources[0]] * 9, src, idx, geo, bc, MEAN, STD, 3)
    with pytest.raises(RuntimeError, match="int32"):
        ops.pool_gather_combined(sources, src.long(), idx, geo, bc, MEAN, STD, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pool_gather_combined(sources, src.cpu(), idx, geo, bc, MEAN, STD, 3)
    with pytest.raises(RuntimeError, match="out img"):
        ops.pool_gather_combined(sources, src, idx, geo, bc, MEAN, STD, 3, out=(
            torch.empty((7, 4, 32, 32), device=DEV), torch.empty((7, 32, 32), dtype=torch.int64, device=DEV),
            torch.empty((7, 32, 32), dtype=torch.int64, device=DEV)))


def test_combined_gather_guard_zeroes_bad_slots_and_flags_them():
    """an index outside ITS source (inside another), a source outside the table, an odd turn of a non-square tile: zeros,
    the matching bit, and the other slots of the batch as usual"""
    from deadtrees_amd import ops
    from deadtrees_amd.data.synthetic import MEAN, STD
    sources = _sources(32, 48)
    _, _, geo, bc = _calls(32, 48)[1]
    good = torch.tensor([0, 1, 2, 4, 5], device=DEV)

    def run(src, idx, geo):
        src = torch.tensor(src, dtype=torch.int32, device=DEV)
        idx = torch.tensor(idx, dtype=torch.int32, device=DEV)
        img, mask, lu, err = ops.pool_gather_combined(sources, src, idx, geo, bc, MEAN, STD, 3, 0)
        for bad in (3, 6):
            assert not img[bad].any() and not mask[bad].any() and not lu[bad].any()
        _assert_slots_equal_single_source((img[good], mask[good], lu[good]), sources, src[good], idx[good], geo[good],
                                          bc[good], 3, 0)
        assert bool(img[good].any())
        return int(err)

    assert run([0, 2, 1, 2, 1, 2, 1], [7, 2, 3, 3, 0, 1, -1], geo) == 1      # idx 3 of source 2 (N = 3); idx -1
    assert run([0, 2, 1, 3, 1, 2, -1], [7, 2, 3, 0, 0, 1, 0], geo) == 4      # sources 3 and -1 of three
    turned = geo.clone()
    turned[3, 1], turned[6, 1] = 1, 3
    assert run(SRC, IDX, turned) == 2                                         # odd turns at 32x48
    assert run([0, 2, 1, 5, 1, 2, 1], [7, 2, 3, 0, 0, 1, 4], turned) == 7    # every bit in one batch


def test_combined_gather_offsets_past_4_gib_in_the_second_source():
    """source 1 holds 2^20 + 4 tiles of 32x32 (4 GiB of image bytes, zeros but for the samples read): samples past 2^31
    and past 2^32 bytes come back right, in one batch with samples of the small source 0"""
    from deadtrees_amd import ops
    from deadtrees_amd.data.synthetic import MEAN, STD
    n, h, w = (1 << 20) + 4, 32, 32
    small = _sources(h, w)[0]
    images = torch.zeros((n, h, w, 4), dtype=torch.uint8, device=DEV)
    masks = torch.zeros((n, h, w), dtype=torch.uint8, device=DEV)
    sums = torch.zeros(n, dtype=torch.int64, device=DEV)
    where = torch.tensor([(1 << 19) + 1, n - 1, 3], device=DEV)
    fill = _sources(h, w)[1]
    images[where], masks[where], sums[where] = fill[0][:3], fill[1][:3], fill[3][:3]
    sources = [(small[0], small[1], None, small[3]), (images, masks, None, sums)]
    src = torch.tensor([1, 0, 1, 1, 0, 1], dtype=torch.int32, device=DEV)
    idx = torch.tensor([n - 1, 8, 3, (1 << 19) + 1, 1, (1 << 19) + 2], dtype=torch.int32, device=DEV)
    geo = torch.tensor([[1, 1], [0, 3], [0, 0], [2, 3], [1, 2], [0, 0]], dtype=torch.int32, device=DEV)
    bc = torch.tensor([[1.1, 0.15], [0.95, 0.1], [1.0, 0.0], [0.9, -0.1], [1.0, 0.0], [1.0, 0.0]], device=DEV)
    img, mask, none, err = ops.pool_gather_combined(sources, src, idx, geo, bc, MEAN, STD, 4, 0)
    assert none is None and int(err) == 0
    _assert_slots_equal_single_source((img, mask, None), sources, src, idx, geo, bc, 4, 0, with_lu=False)
    assert bool(mask[:5].any(dim=2).any(dim=1).all()) and not mask[5].any()
    # index n of the big source is outside it
    idx[0] = n
    assert int(ops.pool_gather_combined(sources, src, idx, geo, bc, MEAN, STD, 4, 0)[3]) == 1
    del images, masks, sources
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ loader and trainer binding
SEED = 5
BS = (3, 1, 2)                                  # batch_size 6 with extras [1, 2]


@pytest.fixture(scope="module")
def shard_dir(tmp_path_factory):
    """main_0..4 (6, 6, 6, 10, 5 samples) -> split (3, 1, 1); neg_0..3 (3 each) and rnd_0..3 (2 each) -> (3, 1); 32x32"""
    d = tmp_path_factory.mktemp("combined")
    rng = np.random.default_rng(9)
    parts = {}
    for name, counts in (("main", (6, 6, 6, 10, 5)), ("neg", (3,) * 4), ("rnd", (2,) * 4)):
        parts[name] = []
        for i, n in enumerate(counts):
            samples = random_samples(rng, n, 32, 32, f"{name}{i}")
            write_shard(d / f"{name}_{i}.tar", samples, compression="tiff_lzw" if i == 1 else None)
            parts[name].append(samples)
    host = {"train": [stack(sum(parts[k][:3], [])) for k in ("main", "neg", "rnd")],
            "val": [stack(parts[k][3]) for k in ("main", "neg", "rnd")], "test": [stack(parts["main"][4])]}
    return str(d), host


def _datamodule(shard_dir):
    from deadtrees_amd.data.deadtreedata import DeadtreesDataModule
    conf = {"batch_size": 6}
    dm = DeadtreesDataModule(shard_dir[0], "main_*.tar", pattern_extra=["neg_*.tar", "rnd_*.tar"], batch_size_extra=[1, 2],
                             train_dataloader_conf=conf, val_dataloader_conf=conf, test_dataloader_conf={"batch_size": 4},
                             device=DEV, seed=SEED)
    dm.setup(in_channels=3, classes=2)
    return dm


def _check_part(item, host, idx, geo, bc, classes=2):
    """one yielded five-tuple against the numpy oracle applied to its rows of the plan, with the caps
    tests/test_pool_gpu.py::_check_batch grants this arithmetic (exact at (1, 0); else <= 1 grey level and < 1 % of
    entries off by more than 1e-3 grey level); labels, lu, stats and distance maps exactly"""
    from deadtrees_amd.data.distmap import distmaps_on_device
    from deadtrees_amd.data.synthetic import MEAN, STD
    from oracle import augment_ref as A
    images, masks, lu, keys, fracs = host
    img, mask, dist, lu_out, stats = item
    n = len(idx)
    assert img.dtype == torch.float32 and tuple(img.shape) == (n, 3, 32, 32) and img.is_contiguous() and img.is_cuda
    assert mask.dtype == torch.int64 and lu_out.dtype == torch.int64 and tuple(mask.shape) == tuple(lu_out.shape) == (n, 32, 32)
    assert dist.dtype == torch.float32 and tuple(dist.shape) == (n, classes, 32, 32)
    assert torch.equal(dist, distmaps_on_device(mask.contiguous(), classes))
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


def _check_batch(batch, hosts, plan, k):
    from deadtrees_amd.data.pool import CombinedBatch
    _, src, idx, geo, bc = plan
    assert isinstance(batch, CombinedBatch) and list(batch) == ["main", "extra_0", "extra_1"]
    whole = batch.combined
    assert tuple(whole[0].shape) == (6, 3, 32, 32) and whole[0].is_contiguous() and len(whole[4]) == 6
    at = 0
    for j, key in enumerate(batch):
        lo = 6 * k + at
        assert src[lo:lo + BS[j]].tolist() == [j] * BS[j]
        _check_part(batch[key], hosts[j], idx[lo:lo + BS[j]], geo[lo:lo + BS[j]], bc[lo:lo + BS[j]])
        for f in range(4):                                   # the parts are views of the combined tensors
            assert batch[key][f].data_ptr() == whole[f][at:at + BS[j]].data_ptr()
        assert batch[key][4] == whole[4][at:at + BS[j]]
        at += BS[j]


def test_combined_loader_epochs_follow_the_plan(shard_dir):
    from deadtrees_amd.data.pool import CombinedPoolLoader, combined_plan
    dm = _datamodule(shard_dir)
    assert {k: len(p) for k, p in dm.pools.items()} == {"train": 18, "val": 10, "test": 5}
    assert [{k: len(p) for k, p in e.items()} for e in dm.extra_pools] == [{"train": 9, "val": 3}, {"train": 6, "val": 2}]
    assert all(p.on_device for e in dm.extra_pools for p in e.values())
    loader = dm.train_dataloader()
    assert isinstance(loader, CombinedPoolLoader) and len(loader) == 9
    epochs = []
    for epoch in range(2):                       # plain iteration: epoch 0, then epoch 1
        batches = list(loader)
        assert loader.epoch == epoch and len(batches) == 9
        plan = combined_plan((18, 9, 6), BS, epoch, SEED, True, True)
        assert plan[0] == 9
        for k, batch in enumerate(batches):
            _check_batch(batch, shard_dir[1]["train"], plan, k)
        epochs.append(batches)
    assert not all(torch.equal(a.combined[0], b.combined[0]) for a, b in zip(*epochs))      # reshuffled, redrawn
    loader.set_epoch(0)
    again = list(loader)
    assert loader.epoch == 0
    for a, b in zip(epochs[0], again):
        assert all(torch.equal(a.combined[i], b.combined[i]) for i in range(4)) and a.combined[4] == b.combined[4]


def test_combined_val_loader_cycles_and_test_loader_is_the_main_set(shard_dir):
    from deadtrees_amd.data.pool import combined_plan
    dm = _datamodule(shard_dir)
    val = dm.val_dataloader()
    assert len(val) == 3                          # main 10 // 3, extra_0 3 // 1, extra_1 2 // 2 = 1: cycled
    plan = combined_plan((10, 3, 2), BS, 0, SEED, False, True)
    for _ in range(2):                            # every epoch alike
        batches = list(val)
        assert len(batches) == 3
        for k, batch in enumerate(batches):
            _check_batch(batch, shard_dir[1]["val"], plan, k)
        assert batches[0]["main"][4] != batches[1]["main"][4]
        for other in batches[1:]:                 # the one batch of extra_1, three times
            assert all(torch.equal(a, b) for a, b in zip(other["extra_1"][:4], batches[0]["extra_1"][:4]))
            assert other["extra_1"][4] == batches[0]["extra_1"][4]
    test = list(dm.test_dataloader())
    assert len(test) == 1 and isinstance(test[0], tuple)          # the bare tuple, at the full batch size of 4
    neutral = (torch.zeros((4, 2), dtype=torch.int32), torch.tensor([[1.0, 0.0]] * 4))
    _check_part(test[0], shard_dir[1]["test"][0], torch.arange(4), *neutral)


def test_combined_loader_feeds_the_captured_step_in_place(shard_dir):
    """fit() on a graph trainer bound to the combined loader: once the step is captured the loader's combined tensors ARE
    the step's static buffers, and create_combined_batch hands them through — no concatenation, no staging copy"""
    from deadtrees_amd.network.segmodel import create_combined_batch
    from deadtrees_amd.network.unet import UNetHIP
    from deadtrees_amd.trainer import HipTrainer, fit
    dm = _datamodule(shard_dir)
    tr = HipTrainer(UNetHIP().to(DEV), graph=True, losses=("GDICE", "FOCAL"))
    loader = dm.train_dataloader(trainer=tr)
    seen = []

    class Recorder:
        def __iter__(self):
            for batch in loader:
                seen.append((batch, tr.static_batch()))
                yield batch

    val = dm.val_dataloader()
    history = fit(tr, Recorder(), epochs=2, val_loader=val)
    assert len(seen) == 18 and [h["epoch"] for h in history] == [0, 1]
    assert all(np.isfinite(h["train/total_loss"]) and np.isfinite(h["val/total_loss"]) for h in history)
    assert all(h["val/samples"] == 18 for h in history)
    for k, (batch, static) in enumerate(seen):
        assert batch.combined[2] is None          # no distance maps: no boundary term asks for them
        if k >= 3:                                # two eager steps, capture on the third, fed in place from the fourth
            assert static is not None
            assert batch.combined[0] is static[0] and batch.combined[1] is static[1]
            assert create_combined_batch(batch)[0] is static[0]
            assert batch["extra_1"][0].data_ptr() == static[0][4:].data_ptr()
        else:
            assert static is None
    last = tr.static_batch()
    replay = dm.train_dataloader()                # unbound: fresh tensors
    replay.set_epoch(1)
    want = list(replay)[-1].combined
    assert torch.equal(last[0], want[0]) and torch.equal(last[1], want[1])


def test_combined_loader_of_one_pool_is_the_pool_loader(shard_dir):
    """the 18-sample train pool alone: both loaders are one implementation and must yield the same epochs"""
    from deadtrees_amd.data.pool import CombinedBatch, CombinedPoolLoader, PoolLoader
    pool = _datamodule(shard_dir).pools["train"]
    b = 4
    kw = dict(train=True, in_channels=3, classes=2, seed=SEED)
    combined, single = CombinedPoolLoader([pool], [b], **kw), PoolLoader(pool, b, **kw)
    assert len(combined) == len(single) == 4
    for epoch in (0, 1):
        pairs = list(zip(combined, single, strict=True))
        assert len(pairs) == 4 and combined.epoch == single.epoch == epoch
        for whole, item in pairs:
            assert isinstance(whole, CombinedBatch) and list(whole) == ["main"] and list(item) == ["main"]
            for f in range(4):
                assert tuple(whole.combined[f].shape)[0] == b and torch.equal(whole.combined[f], item["main"][f])
            assert whole.combined[4] == item["main"][4] and len(item["main"][4]) == b
