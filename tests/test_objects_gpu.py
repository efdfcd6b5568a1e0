"""Crown-level validation curves on the device (``csrc/objects.hip`` through ``ops.object_histogram``) against the numpy
oracle of ``loss/objects.py`` with ``array_equal`` — every count is an integer —, then ``HipTrainer.validate(objects=...)``,
its captured graph and ``fit(objects=...)``.

The shapes: odd sizes (19 x 33: no image row starts on an 8- or 16-byte boundary), a size of whole 4-pixel groups (64 x 64),
a single pixel, batch sizes that fill the plane's grid of cells (1), leave an empty cell (3 in 2 x 2) and need a third
column (5), and one plane of more than 65,537 pixels per patch (the sum of q passes 32 bits)."""
import numpy as np
import pytest
import torch

import objects_cases as oc
from deadtrees_amd import ops
from deadtrees_amd.loss.objects import ObjectCurves, ObjectSweep, object_histogram_host

pytestmark = pytest.mark.gpu
DEV = "cuda"
Q = 40000
J = Q >> 8


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _device(q, target, sweep, **kw):
    hist, targets, err = ops.object_histogram(_dev(q), _dev(target), sweep, **kw)
    assert hist.dtype == torch.int64 and tuple(hist.shape) == (q.shape[1], 2, 256, 256)
    assert targets.dtype == torch.int64 and tuple(targets.shape) == (q.shape[1],) and err.dtype == torch.int32
    return hist.cpu().numpy(), targets.cpu().numpy(), int(err.cpu())


def _same(got, want):
    assert np.array_equal(got[0], want[0]), (np.argwhere(got[0] != want[0])[:8], got[0].sum(), want[0].sum())
    assert np.array_equal(got[1], want[1]), (got[1], want[1])
    assert got[2] == want[2]


def _sweeps(K):
    for connectivity in (4, 8):
        for min_pixels in (0, 4):
            for min_iou in (0.5, 0.75):
                yield ObjectSweep.from_q(oc.low_for(K), connectivity=connectivity, min_pixels=min_pixels, min_iou=min_iou)


@pytest.mark.parametrize("K", [2, 3, 8])
@pytest.mark.parametrize("size", [(19, 33), (64, 64), (1, 1)], ids=["19x33", "64x64", "1x1"])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_device_equals_the_host(B, size, K):
    q, target = oc.blobs(oc.CLOSURE_SEEDS.get(K, K) if (B, size) == (3, (19, 33)) else 7 * B + K, B, K, *size)
    patches = matches = 0
    for sweep in _sweeps(K):
        want = object_histogram_host(q, target, sweep)
        _same(_device(q, target, sweep), want)
        patches, matches = patches + int(want[0].sum()), matches + int(want[0][:, 1].sum())
    if size != (1, 1):
        assert patches > 0 and matches > 0                       # never vacuous
    if (B, size) == (3, (19, 33)) and K in oc.CLOSURE_SEEDS:    # the closure inputs: found, invented and missed crowns
        sweep = ObjectSweep.from_q(oc.low_for(K))
        cv = ObjectCurves(*object_histogram_host(q, target, sweep)[:2], sweep)
        for c in range(1, K):
            assert min(int(v[-(-sweep.low[c] // 256)]) for v in cv.counts(c)) >= 1


def test_views_that_start_off_every_wide_load():
    """q and the target as views one image into a larger tensor of odd planes: no 8- or 16-byte alignment anywhere"""
    q, target = oc.blobs(21, 4, 3, 19, 33)
    sweep = ObjectSweep.from_q(oc.low_for(3), min_pixels=2)
    hist, targets, err = ops.object_histogram(_dev(q)[1:], _dev(target)[1:], sweep)
    want = object_histogram_host(q[1:], target[1:], sweep)
    _same((hist.cpu().numpy(), targets.cpu().numpy(), int(err.cpu())), want)
    assert want[0].sum() > 0


def _full(B, K, H, W, pred_class=1):
    q = np.zeros((B, K, H, W), dtype=np.uint16)
    q[:, pred_class] = Q
    return q


@pytest.mark.parametrize("connectivity", [4, 8])
def test_nothing_joins_or_matches_across_image_borders(connectivity):
    """every image full: patches touch all four borders on both sides of every gutter, diagonal neighbours included"""
    sweep = ObjectSweep.from_q({1: 20000}, connectivity=connectivity)
    H, W = 6, 10
    for B in (2, 3, 4, 5, 9):
        q, target = _full(B, 2, H, W), np.ones((B, H, W), dtype=np.int64)
        got = _device(q, target, sweep)
        _same(got, object_histogram_host(q, target, sweep))
        assert got[0][1, 1, J, J] == B and got[0].sum() == B and got[1][1] == B
    # the same pixels split differently over the images: one crown that spans the cut is one match in the whole plane, two
    # crowns in two half planes; a prediction on one side of the cut cannot reach the target on the other
    q = np.zeros((1, 2, H, 2 * W), dtype=np.uint16)
    target = np.zeros((1, H, 2 * W), dtype=np.int64)
    q[0, 1, 1:5, W - 4:W] = Q                                    # the prediction: left of the cut only
    target[0, 1:5, W - 3:W + 1] = 1                              # the crown: three columns left, one right
    whole = _device(q, target, sweep)
    _same(whole, object_histogram_host(q, target, sweep))
    assert whole[0][1, 1, J, J] == 1 and whole[1][1] == 1        # 12 of 20 pixels: a match
    q2 = np.ascontiguousarray(np.stack([q[0, :, :, :W], q[0, :, :, W:]]))
    t2 = np.ascontiguousarray(np.stack([target[0, :, :W], target[0, :, W:]]))
    split = _device(q2, t2, sweep)
    _same(split, object_histogram_host(q2, t2, sweep))
    assert split[0][1, 1, J, J] == 1 and split[1][1] == 2        # 12 of 16: still a match; the sliver is a crown of its own
    # rows: the same with the cut between an image and the one below it in the plane (B = 3: images 0 and 2)
    q3, t3 = np.zeros((3, 2, H, W), dtype=np.uint16), np.zeros((3, H, W), dtype=np.int64)
    q3[0, 1, H - 2:, 2:6] = Q
    t3[2, :2, 2:6] = 1
    rows = _device(q3, t3, sweep)
    _same(rows, object_histogram_host(q3, t3, sweep))
    assert rows[0][1, 0, J, J] == 1 and rows[0].sum() == 1 and rows[1][1] == 1


def test_one_patch_over_every_image():
    """contention on one vote word per image, and sums of q past 32 bits: 264 x 264 pixels at q = 65535"""
    B, H, W = 3, 264, 264
    q = np.zeros((B, 3, H, W), dtype=np.uint16)
    q[:, 1] = 65535
    assert H * W * 65535 > 2 ** 32
    sweep = ObjectSweep.from_q({1: 20000, 2: 20000})
    itself = np.ones((B, H, W), dtype=np.int64)
    got = _device(q, itself, sweep)
    _same(got, object_histogram_host(q, itself, sweep))
    assert got[0][1, 1, 255, 255] == B and got[0].sum() == B and np.array_equal(got[1], [0, B, 0])
    halves = np.ones((B, H, W), dtype=np.int64)
    halves[:, :, W // 2:] = 2                                    # two crowns per image; the class-1 half is exactly 1/2
    got = _device(q, halves, sweep)
    _same(got, object_histogram_host(q, halves, sweep))
    assert got[0][1, 0, 255, 255] == B and got[0].sum() == B and np.array_equal(got[1], [0, B, B])
    halves[:, :, W // 2] = 1                                     # one column more: above 1/2
    got = _device(q, halves, sweep)
    _same(got, object_histogram_host(q, halves, sweep))
    assert got[0][1, 1, 255, 255] == B and got[0].sum() == B


def test_a_checkerboard_against_a_full_target():
    H = W = 64
    board = (np.add.outer(np.arange(H), np.arange(W)) % 2).astype(bool)
    q = np.zeros((2, 2, H, W), dtype=np.uint16)
    q[:, 1] = np.where(board, Q, 0)
    q[1, 1] = np.where(board, 0, 30000)                          # the other colour in the second image
    target = np.ones((2, H, W), dtype=np.int64)
    four = ObjectSweep.from_q({1: 20000}, connectivity=4)
    got = _device(q, target, four)
    _same(got, object_histogram_host(q, target, four))
    assert got[0][1, 0].sum() == H * W and got[0][1, 1].sum() == 0 and got[1][1] == 2      # 4096 single pixels, no match
    eight = ObjectSweep.from_q({1: 20000}, connectivity=8)
    got = _device(q, target, eight)
    _same(got, object_histogram_host(q, target, eight))
    assert got[0].sum() == 2 and got[0][1, 0].sum() == 2          # one patch per image at an IoU of exactly 1/2


def test_empty_planes():
    sweep = ObjectSweep.from_q({1: 20000, 2: 20000})
    q, target = oc.blobs(4, 3, 3, 19, 33)
    nothing = np.zeros_like(q)
    got = _device(nothing, target, sweep)
    _same(got, object_histogram_host(nothing, target, sweep))
    assert got[0].sum() == 0 and got[1].sum() > 0
    empty = np.zeros_like(target)
    got = _device(q, empty, sweep)
    _same(got, object_histogram_host(q, empty, sweep))
    assert got[0].sum() > 0 and got[0][:, 1].sum() == 0 and got[1].sum() == 0
    got = _device(nothing, empty, sweep)
    assert got[0].sum() == 0 and got[1].sum() == 0 and got[2] == 0


def test_a_bad_label_sets_err_and_changes_nothing_else():
    q, target = oc.blobs(oc.CLOSURE_SEEDS[3], 3, 3, 19, 33)
    sweep = ObjectSweep.from_q(oc.low_for(3))
    bad = target.copy()
    at = np.argwhere(target == 0)[[0, 5, 11, 17]]
    for (b, y, x), v in zip(at, (3, -1, 2 ** 40, 255)):
        bad[b, y, x] = v
    clean, flagged = _device(q, target, sweep), _device(q, bad, sweep)
    assert clean[2] == 0 and flagged[2] == 1
    assert np.array_equal(clean[0], flagged[0]) and np.array_equal(clean[1], flagged[1])
    _same(flagged, object_histogram_host(q, bad, sweep))


def test_repeated_calls_add():
    q, target = oc.blobs(oc.CLOSURE_SEEDS[2], 3, 2, 19, 33)
    q2, target2 = oc.blobs(9, 5, 2, 64, 64)
    sweep = ObjectSweep.from_q(oc.low_for(2))
    a, b = object_histogram_host(q, target, sweep), object_histogram_host(q2, target2, sweep)
    hist, targets, err = ops.object_histogram(_dev(q), _dev(target), sweep)
    again = ops.object_histogram(_dev(q2), _dev(target2), sweep, hist=hist, targets=targets, err=err)
    assert again[0] is hist and again[1] is targets and again[2] is err
    ops.object_histogram(_dev(q), _dev(target), sweep, hist=hist, targets=targets, err=err)
    assert np.array_equal(hist.cpu().numpy(), 2 * a[0] + b[0]) and np.array_equal(targets.cpu().numpy(), 2 * a[1] + b[1])
    assert int(err.cpu()) == 0


def test_bad_arguments_raise_before_any_launch():
    q, target = oc.blobs(1, 2, 2, 8, 8)
    sweep = ObjectSweep.from_q({1: 20000})
    dq, dt = _dev(q), _dev(target)
    with pytest.raises(RuntimeError, match="uint16"):
        ops.object_histogram(dq.float(), dt, sweep)
    with pytest.raises(RuntimeError, match="uint16"):
        ops.object_histogram(dq[0], dt, sweep)
    with pytest.raises(RuntimeError, match="uint16"):
        ops.object_histogram(dq[:, :, :, ::2], dt[:, :, ::2].contiguous(), sweep)      # not contiguous
    with pytest.raises(RuntimeError, match="target must be"):
        ops.object_histogram(dq, dt.int(), sweep)
    with pytest.raises(RuntimeError, match="target must be"):
        ops.object_histogram(dq, dt[:, :, :4].contiguous(), sweep)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.object_histogram(dq.cpu(), dt.cpu(), sweep)
    with pytest.raises(ValueError, match="ObjectSweep"):
        ops.object_histogram(dq, dt, {1: 20000})
    with pytest.raises(ValueError, match="K=2"):
        ops.object_histogram(dq, dt, ObjectSweep.from_q({1: 20000, 2: 20000}))
    with pytest.raises(RuntimeError, match="hist must be"):
        ops.object_histogram(dq, dt, sweep, hist=torch.zeros((2, 2, 256, 255), dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match="targets must be"):
        ops.object_histogram(dq, dt, sweep, targets=torch.zeros(3, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match="err must be"):
        ops.object_histogram(dq, dt, sweep, err=torch.zeros(1, dtype=torch.int64, device=DEV))
    # planes beyond the labeller's limits: a side above 16384
    wide = torch.zeros((1, 2, 1, 16384), dtype=torch.uint16, device=DEV)
    with pytest.raises(RuntimeError, match="sides must be <= 16384"):
        ops.object_histogram(wide, torch.zeros((1, 1, 16384), dtype=torch.int64, device=DEV), sweep)
    assert ops.object_plane_shape(5, 8191, 1)[1] == 16384
    tall = torch.zeros((7, 2, 8191, 1), dtype=torch.uint16, device=DEV)          # 3 rows of cells
    with pytest.raises(RuntimeError, match="sides must be <= 16384"):
        ops.object_histogram(tall, torch.zeros((7, 8191, 1), dtype=torch.int64, device=DEV), sweep)
    for B, H, W in ((1, 1, 1), (3, 19, 33), (5, 64, 64), (32, 512, 512)):        # the layout holds every image and a gutter
        cols, ph, pw = ops.object_plane_shape(B, H, W)
        assert cols * (-(-B // cols)) >= B and ph == -(-B // cols) * (H + 1) and pw >= cols * (W + 1) and pw % 4 == 0


# ---------------------------------------------------------------------- validation
SWEEP = ObjectSweep({1: 0.3}, min_pixels=2)


def _hand_objects(model, batches, precision="fp32", sweep=SWEEP):
    hist = np.zeros((2, 2, 256, 256), dtype=np.int64)
    targets = np.zeros(2, dtype=np.int64)
    for img, mask, _, lu in batches:
        _, err, q = ops.prob_histogram(model.predict_logits(img, precision=precision), mask, lu, logits=True, want_q=True)
        h, t, e = object_histogram_host(q.cpu().numpy(), mask.cpu().numpy(), sweep)
        assert int(err.cpu()) == 0 and e == 0
        hist, targets = hist + h, targets + t
    return ObjectCurves(hist, targets, sweep)


def _same_epoch(val, ref):
    assert set(val) == set(ref)
    for k in ref:
        if k.startswith("cm_"):
            assert torch.equal(val[k], ref[k]), k
        elif k == "curves":
            assert val[k] == ref[k]
        else:
            assert val[k] == ref[k], k


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_validate_with_objects(precision):
    import test_validate_gpu as tv
    tr = tv._trainer(precision)
    batches = tv._batches()
    want = _hand_objects(tr.model, batches, precision)
    assert want.hist.sum() > 0 and want.targets[1] > 0           # there are patches and crowns to count
    with_curves = tr.validate(batches, alpha=tv.ALPHA, curves=True)
    val = tr.validate(batches, alpha=tv.ALPHA, curves=True, objects=SWEEP)
    got = val.pop("objects")
    assert isinstance(got, ObjectCurves) and got == want and got.sweep == SWEEP
    _same_epoch(val, with_curves)                                # every other entry is the curves=True epoch
    only = tr.validate(batches, alpha=tv.ALPHA, objects=SWEEP)   # without curves: the same chain, a throw-away histogram
    assert only.pop("objects") == want and "curves" not in only
    with_curves.pop("curves")
    _same_epoch(only, with_curves)
    # an epoch without objects in between leaves nothing behind; the next one with objects starts from zero
    between = tr.validate(batches, alpha=tv.ALPHA)
    assert "objects" not in between and "curves" not in between
    assert tr.validate(batches, alpha=tv.ALPHA, objects=SWEEP)["objects"] == want
    other = ObjectSweep({1: 0.3}, connectivity=4)
    assert tr.validate(batches, alpha=tv.ALPHA, objects=other)["objects"] == _hand_objects(tr.model, batches, precision, other)
    for bad in (True, {1: 0.3}, ObjectSweep({1: 0.3, 2: 0.3})):
        with pytest.raises(ValueError, match="validate: objects"):
            tr.validate(batches, objects=bad)
    s = got.summary()
    assert s["val/crown_targets_1"] == float(want.targets[1]) and 0.0 < s["val/crown_best_threshold_1"] < 1.0


def test_validate_with_objects_replays_a_captured_graph():
    import test_validate_gpu as tv
    tr = tv._trainer(graph=True)
    batches = tv._batches()
    want = _hand_objects(tr.model, batches)
    plain = tr.validate(batches)                                 # the fused path keeps its own graphs
    plain_keys = set(tr._val_replays.keys())
    for epoch in range(4):                                       # eager warm-up, the capture, replays
        val = tr.validate(batches, objects=SWEEP)
        assert val["objects"] == want, epoch
        assert torch.equal(val["cm_px"], plain["cm_px"]) and val["val/dice"] == plain["val/dice"]
    new_keys = set(tr._val_replays.keys()) - plain_keys           # the sweep is part of the key
    assert plain_keys and len(new_keys) == len(plain_keys)
    assert all(k[-1] == ("objects",) + SWEEP._key() for k in new_keys)
    assert all(r.captured for k, r in zip(tr._val_replays.keys(), tr._val_replays.values()) if k in new_keys)
    # another sweep is another graph; the plain epoch still replays its own and returns what it returned
    other = ObjectSweep({1: 0.3}, connectivity=4)
    assert tr.validate(batches, objects=other)["objects"] == _hand_objects(tr.model, batches, sweep=other)
    assert len(set(tr._val_replays.keys()) - plain_keys) == 2 * len(plain_keys)
    again = tr.validate(batches)
    assert "objects" not in again and again["val/dice"] == plain["val/dice"] and torch.equal(again["cm_px"], plain["cm_px"])


def test_fit_logs_the_crown_scalars_and_monitors_them(tmp_path):
    import test_validate_gpu as tv
    from deadtrees_amd.trainer import CheckpointConfig, fit
    tr = tv._trainer()
    train = [(img, mask, None, None, None) for img, mask, _, _ in tv._batches((2, 2), first_seed=80)]
    ck = CheckpointConfig(str(tmp_path / "ck"), monitor="val/crown_best_f1_1", mode="max")
    history = fit(tr, train, epochs=2, val_loader=tv._batches(), objects=SWEEP, checkpoint=ck)
    want = tr.validate(tv._batches(), alpha=min(2 * 0.01, 0.99), objects=SWEEP)["objects"].summary("val")
    for record in history[:-1]:
        assert "objects" not in record and "curves" not in record and not any(k.startswith("cm_") for k in record)
        assert set(want) <= set(record) and "val/dice" in record
    assert {k: history[-2][k] for k in want} == want
    assert history[-1]["checkpoint/best_model_score"] == max(r["val/crown_best_f1_1"] for r in history[:-1])
    with pytest.raises(ValueError, match="not a validation metric"):
        fit(tv._trainer(), train, epochs=1, val_loader=tv._batches(), checkpoint=ck)
    with pytest.raises(ValueError, match="val_loader"):
        fit(tv._trainer(), train, epochs=1, objects=SWEEP)
    with pytest.raises(ValueError, match=r"fit\(objects=...\): objects must be an ObjectSweep"):
        fit(tv._trainer(), train, epochs=1, val_loader=tv._batches(), objects=True)
    plain = fit(tv._trainer(), train, epochs=1, val_loader=tv._batches())
    assert not any("crown" in k for k in plain[0])
