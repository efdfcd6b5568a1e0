"""Operating points on the device (``csrc/curves.hip``): ``ops.prob_histogram`` and ``ops.decide_classes`` against the
numpy oracle of ``loss/curves.py`` with ``array_equal`` — every count is an integer —, the K = 2 closure between the
curves and the decided maps, ``HipTrainer.validate(curves=True)`` and ``infer_tile(decision=...)``.

The shapes come from ``ops.CURVE_CHUNK``: more than two chunks, a pixel count that is no multiple of 4, a chunk that
straddles two images, and planes whose offsets are no multiple of 16 bytes (odd ``H * W``)."""
import math

import numpy as np
import pytest
import torch

from deadtrees_amd import ops
from deadtrees_amd.loss.curves import (BINS, Decision, ProbabilityCurves, decide_host, prob_histogram_host, q_histogram_host,
                                       quantise)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _big_shape():
    """(B, K, H, W) = (3, 2, s, s) with s odd and 3 s^2 just above two chunks"""
    C = ops.CURVE_CHUNK
    s = math.isqrt(2 * C // 3) + 1
    s += 1 - s % 2
    assert s % 2 == 1 and 3 * s * s > 2 * C and (3 * s * s) % 4 != 0            # > 2 chunks, ragged, odd planes
    assert s * s < C < 2 * s * s                                                # chunk 0 ends inside image 1
    return 3, 2, s, s


def _realistic(rng, B, K, H, W):
    """about 97 % confident background, the rest spread over the classes"""
    p = np.full((B, K, H, W), 0.002 / max(K - 1, 1), dtype=np.float32)
    p[:, 0] = 0.998
    dead = rng.random((B, H, W)) < 0.03
    soft = rng.random((B, K, H, W)).astype(np.float32)
    soft /= soft.sum(1, keepdims=True)
    return np.where(dead[:, None], soft, p).astype(np.float32), np.where(dead, rng.integers(1, K, (B, H, W)), 0)


def _case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    shape = {"big": _big_shape(), "mid": (2, 3, 37, 53), "wide": (1, 8, 16, 20)}[name.split(",")[0]]
    B, K, H, W = shape
    kind = name.split(",")[1].strip()
    lu = rng.integers(0, 3, (B, H, W))
    labels = rng.integers(0, K, (B, H, W))
    if kind == "realistic":
        p, labels = _realistic(rng, B, K, H, W)
    elif kind == "uniform":
        p = rng.random((B, K, H, W)).astype(np.float32)
    elif kind == "one counter":                                  # every pixel lands in one counter per class and plane
        p = np.zeros((B, K, H, W), dtype=np.float32)
        p[:, 0] = 1.0
        labels, lu = np.zeros((B, H, W), dtype=np.int64), np.ones((B, H, W), dtype=np.int64)
    elif kind == "odd values":
        p = rng.random((B, K, H, W)).astype(np.float32)
        flat = p.reshape(-1)
        idx = rng.permutation(flat.size)[:flat.size // 4]
        flat[idx] = rng.choice(np.array([np.nan, -0.5, 1.5, np.inf, -np.inf, 0.0, 1.0], dtype=np.float32), idx.size)
    elif kind == "bad labels":
        p = rng.random((B, K, H, W)).astype(np.float32)
        labels.reshape(-1)[rng.permutation(labels.size)[:7]] = np.array([K, -1, K + 5, 255, -2 ** 40, 2 ** 40, K])
    else:
        raise KeyError(kind)
    return p, labels.astype(np.int64), lu.astype(np.int64)


CASES = ["big, realistic", "big, uniform", "big, one counter", "big, odd values", "big, bad labels",
         "mid, realistic", "mid, uniform", "mid, one counter", "mid, odd values", "mid, bad labels",
         "wide, realistic", "wide, uniform", "wide, one counter", "wide, odd values", "wide, bad labels"]


@pytest.mark.parametrize("with_lu", [True, False], ids=["lu", "no lu"])
@pytest.mark.parametrize("name", CASES)
def test_probability_histogram_equals_the_host(name, with_lu):
    p, labels, lu = _case(name)
    lu = lu if with_lu else None
    want, want_err = prob_histogram_host(p, labels, lu)
    hist, err, q = ops.prob_histogram(_dev(p), _dev(labels), _dev(lu), want_q=True)
    assert hist.dtype == torch.int64 and tuple(hist.shape) == (2, p.shape[1], 2, BINS) and q.dtype == torch.uint16
    assert np.array_equal(hist.cpu().numpy(), want)
    assert int(err.cpu()) == want_err == int("bad labels" in name)
    assert np.array_equal(q.cpu().numpy().astype(np.int64), quantise(p))         # out-of-range pixels included
    if "one counter" in name:
        n = labels.size
        assert want[0, 0, 1, 255] == n and want[0, 1, 0, 0] == n and (want[1] == want[0]).all() == with_lu
    if not with_lu:
        assert want[1].sum() == 0
    # a given histogram is added to, not overwritten; so is the flag
    again, err2 = ops.prob_histogram(_dev(p), _dev(labels), _dev(lu), hist=hist, err=err)
    assert again is hist and err2 is err and np.array_equal(hist.cpu().numpy(), 2 * want) and int(err.cpu()) == want_err


def test_views_offsets_and_bad_arguments():
    rng = np.random.default_rng(7)
    B, K, H, W = 3, 3, 9, 11                                     # 99 pixels per plane: slices start off the 16-byte grid
    p = rng.random((B + 1, K, H, W)).astype(np.float32)
    labels, lu = rng.integers(0, K, (B + 1, H, W)), rng.integers(0, 2, (B + 1, H, W))
    want, _ = prob_histogram_host(p[1:], labels[1:], lu[1:])
    hist, err, q = ops.prob_histogram(_dev(p)[1:], _dev(labels)[1:], _dev(lu)[1:], want_q=True)
    assert np.array_equal(hist.cpu().numpy(), want) and int(err.cpu()) == 0
    assert np.array_equal(q.cpu().numpy().astype(np.int64), quantise(p[1:]))
    hist32, _ = ops.prob_histogram(_dev(p)[1:], _dev(labels.astype(np.int32))[1:], _dev(lu.astype(np.uint8))[1:])
    assert np.array_equal(hist32.cpu().numpy(), want)            # other integer types are converted
    with pytest.raises(RuntimeError, match="same number of pixels"):
        ops.prob_histogram(_dev(p), _dev(labels[1:]))
    with pytest.raises(RuntimeError, match="same number of pixels"):
        ops.prob_histogram(_dev(p), _dev(labels), _dev(lu[:, :4]))
    with pytest.raises(RuntimeError, match="hist must be"):
        ops.prob_histogram(_dev(p), _dev(labels), hist=torch.zeros((2, K, 2, 255), dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match="float32"):
        ops.prob_histogram(_dev(p.astype(np.float64)), _dev(labels))
    with pytest.raises(RuntimeError, match="K=9"):
        ops.prob_histogram(torch.zeros((1, 9, 4, 4), device=DEV), torch.zeros((1, 4, 4), dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.prob_histogram(torch.zeros((1, 2, 4, 4)), torch.zeros((1, 4, 4), dtype=torch.int64))
    assert isinstance(ops.CURVE_CHUNK, int) and ops.CURVE_CHUNK % 1024 == 0


@pytest.mark.parametrize("scale", [1.0, 4.0, 12.0])
@pytest.mark.parametrize("K", [2, 3, 8])
def test_logits_mode(K, scale):
    """the histogram is exactly that of the device's own q; its q is within one step of the float64 softmax's: an fp32
    softmax error of a few 1e-7 relative moves p * 65535 by less than 0.05, so only the floor's boundary can flip"""
    rng = np.random.default_rng(100 * K + int(scale))
    B, H, W = 2, 37, 53
    z = (rng.standard_normal((B, K, H, W)) * scale).astype(np.float32)
    labels, lu = rng.integers(0, K, (B, H, W)), rng.integers(0, 2, (B, H, W))
    hist, err, q = ops.prob_histogram(_dev(z), _dev(labels), _dev(lu), logits=True, want_q=True)
    q = q.cpu().numpy().astype(np.int64)
    assert np.array_equal(hist.cpu().numpy(), q_histogram_host(q, labels, lu)[0]) and int(err.cpu()) == 0
    z64 = z.astype(np.float64)
    e = np.exp(z64 - z64.max(1, keepdims=True))
    q64 = quantise((e / e.sum(1, keepdims=True)).astype(np.float32))
    diff = np.abs(q - q64)
    share = float((diff != 0).mean())
    print(f"K={K} scale={scale}: max |q - q64| = {int(diff.max())}, share differing = {share:.5f}")
    assert diff.max() <= 1
    assert share <= 0.01
    assert hist.cpu().numpy()[0].sum() == K * B * H * W


@pytest.mark.parametrize("K", [2, 3, 8])
def test_decide_classes_equals_the_host(K):
    rng = np.random.default_rng(K)
    h, w = 37, 53                                                # 1961 pixels: two blocks, a ragged tail, odd planes
    assert (h * w) % 4 != 0 and h * w > 1024
    p = (rng.integers(0, 9, (K, h, w)) / 8.0).astype(np.float32)   # coarse values: many equal q among the classes
    p[:, 0, :7] = np.array([np.nan, -1.0, 2.0, 0.0, 1.0, 0.5, 0.25], dtype=np.float32)
    decision = Decision.from_q({c: int(quantise(np.float32(0.125 * (1 + c % 4)))) for c in range(1, K)})
    want = decide_host(p, decision)
    if K > 2:
        q = quantise(p[1:])
        top = q.max(0)
        assert (((q == top) & (q >= decision.thresholds_u16()[1:, None, None])).sum(0) > 1).any()      # real ties
    got = ops.decide_classes(_dev(p), decision)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (h, w) and np.array_equal(got.cpu().numpy(), want)
    assert len(np.unique(want)) == K
    # thresholds as integers, an output buffer, and a view that starts off the 16-byte grid
    out = torch.full((h, w), 255, dtype=torch.uint8, device=DEV)
    assert ops.decide_classes(_dev(p), [0] + [decision.q[c] for c in range(1, K)], out=out) is out
    assert np.array_equal(out.cpu().numpy(), want)
    flat = _dev(np.concatenate([np.zeros(3, dtype=np.float32), p.reshape(-1)]))[3:].view(K, h, w)
    assert np.array_equal(ops.decide_classes(flat, decision).cpu().numpy(), want)
    with pytest.raises(ValueError):
        ops.decide_classes(_dev(p), Decision.from_q({c: 5 for c in range(1, K + 1)}))
    with pytest.raises(ValueError):
        ops.decide_classes(_dev(p), [0] * K)
    with pytest.raises(RuntimeError):
        ops.decide_classes(_dev(p), decision, out=torch.zeros((h, w + 1), dtype=torch.uint8, device=DEV))


@pytest.mark.parametrize("j", [1, 77, 128, 255])
def test_k2_closure_on_the_device(j):
    rng = np.random.default_rng(11)
    B, H, W = 3, 41, 59
    p = rng.random((B, 2, H, W)).astype(np.float32) ** 2
    p[:, 0] = 1 - p[:, 1]
    labels, lu = rng.integers(0, 2, (B, H, W)), rng.integers(0, 2, (B, H, W))
    hist, _ = ops.prob_histogram(_dev(p), _dev(labels), _dev(lu))
    cv = ProbabilityCurves(hist.cpu().numpy())
    decision = Decision.from_q({1: 256 * j})
    decided = np.stack([ops.decide_classes(_dev(p[b]), decision).cpu().numpy() for b in range(B)])
    for masked in (False, True):
        sel = (lu == 1) if masked else np.ones(lu.shape, dtype=bool)
        tp, fp, fn, tn = (int(v[j]) for v in cv.counts(1, masked))
        assert tp == int(((decided == 1) & (labels == 1) & sel).sum()) and fp == int(((decided == 1) & (labels == 0) & sel).sum())
        assert fn == int(((decided == 0) & (labels == 1) & sel).sum()) and tn == int(((decided == 0) & (labels == 0) & sel).sum())


# ---------------------------------------------------------------------- validation
def _hand_histogram(model, batches, precision="fp32"):
    hist = None
    for img, mask, _, lu in batches:
        hist, err = ops.prob_histogram(model.predict_logits(img, precision=precision), mask, lu, hist=hist, logits=True)
        assert int(err.cpu()) == 0
    return hist.cpu().numpy()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_validate_with_curves(precision):
    import test_validate_gpu as tv
    tr = tv._trainer(precision)
    batches = tv._batches()
    plain = tr.validate(batches, alpha=tv.ALPHA)
    val = tr.validate(batches, alpha=tv.ALPHA, curves=True)
    cv = val.pop("curves")
    assert isinstance(cv, ProbabilityCurves) and cv.K == tv.K
    assert np.array_equal(cv.hist, _hand_histogram(tr.model, batches, precision))
    assert cv.hist[0, 1].sum() == sum(tv.SIZES) * 64 * 64 and 0 < cv.hist[1, 1].sum() < cv.hist[0, 1].sum()
    # the arg-max point of the confusion matrix is one point of the curves' data: positives and pixels agree
    assert int(cv.counts(1)[0][0]) == int(plain["cm_px"][1].sum())
    assert int(cv.counts(1, masked=True)[0][0]) == int(plain["cm_px_masked"][1].sum())
    # the scalar metrics are those of the fused path: F-scores and matrices equal, loss terms to fp32 summation order (the
    # tolerance of tests/test_validate_gpu.py::_compare)
    assert set(val) == set(plain)
    assert val["val/dice"] == plain["val/dice"] and val["val/dice_with_bg"] == plain["val/dice_with_bg"]
    for name in ("cm_px", "cm_norm", "cm_px_masked", "cm_norm_masked"):
        assert torch.equal(val[name], plain[name]), name
    for key in ("val/total_loss", "val/dice_loss", "val/focal_loss"):
        assert val[key] == pytest.approx(plain[key], rel=1e-5, abs=1e-6), key
    assert val["val/batches"] == plain["val/batches"] and val["val/samples"] == plain["val/samples"]
    # an epoch without curves in between leaves nothing behind; the next one with curves starts from zero
    assert "curves" not in tr.validate(batches, alpha=tv.ALPHA)
    assert tr.validate(batches, alpha=tv.ALPHA, curves=True)["curves"] == cv
    s = cv.summary()
    assert 0.0 <= s["val/ap_1"] <= 1.0 and 0.0 <= s["val/roc_auc_1"] <= 1.0 and 0.0 < s["val/best_threshold_1"] < 1.0


def test_validate_with_curves_replays_a_captured_graph():
    import test_validate_gpu as tv
    tr = tv._trainer(graph=True)
    batches = tv._batches()
    want = _hand_histogram(tr.model, batches)
    plain = tr.validate(batches)                                 # the fused path keeps its own graphs
    plain_keys = set(tr._val_replays.keys())
    for epoch in range(4):                                       # eager warm-up, the capture, replays
        val = tr.validate(batches, curves=True)
        assert np.array_equal(val["curves"].hist, want), epoch
        assert torch.equal(val["cm_px"], plain["cm_px"]) and val["val/dice"] == plain["val/dice"]
    new_keys = set(tr._val_replays.keys()) - plain_keys           # the flag is part of the key
    assert plain_keys and len(new_keys) == len(plain_keys) and all(k[-1] is True for k in new_keys)
    assert all(r.captured for k, r in zip(tr._val_replays.keys(), tr._val_replays.values()) if k in new_keys)


def test_fit_logs_the_curve_scalars():
    import test_validate_gpu as tv
    from deadtrees_amd.trainer import fit
    tr = tv._trainer()
    train = [(img, mask, None, None, None) for img, mask, _, _ in tv._batches((2, 2), first_seed=80)]
    history = fit(tr, train, epochs=2, val_loader=tv._batches(), curves=True)
    want = tr.validate(tv._batches(), alpha=min(2 * 0.01, 0.99), curves=True)["curves"].summary("val")
    for record in history:
        assert "curves" not in record and not any(k.startswith("cm_") for k in record)
        assert {"val/ap_1", "val/roc_auc_1", "val/best_f1_1", "val/best_threshold_1", "val/dice"} <= set(record)
    assert {k: history[-1][k] for k in want} == want
    plain = fit(tv._trainer(), train, epochs=1, val_loader=tv._batches())
    assert not any("ap_" in k or "threshold" in k for k in plain[0])


# ---------------------------------------------------------------------- inference
@pytest.fixture(scope="module")
def inference(tmp_path_factory):
    from deadtrees_amd.deployment.inference import PyTorchInference
    from deadtrees_amd.network.segmodel import SemSegment
    from deadtrees_amd.utils.config import default_network, default_training
    from oracle.unet_ref import make_oracle
    model = SemSegment(default_network(in_channels=3), default_training())
    model.model.load_state_dict(make_oracle(3, 2, seed=3).state_dict())
    file = tmp_path_factory.mktemp("ckpt") / "bestmodel.ckpt"
    model.save_checkpoint(file)
    return PyTorchInference(file)


def test_infer_tile_with_a_decision(inference):
    from deadtrees_amd.deployment.attributes import AttributeConfig, patch_attributes_host
    from deadtrees_amd.deployment.patches import PatchConfig, labelled_patches_host
    from deadtrees_amd.deployment.tiler import infer_rasters, infer_tile
    raster = np.random.default_rng(31).integers(0, 256, (3, 200, 232), dtype=np.uint8)
    kw = dict(subtile=128, overlap=64, blend="average", device=DEV, batch_size=4)
    plain_map, probs = infer_tile(inference, raster, return_probs=True, **kw)
    none_map, none_probs = infer_tile(inference, raster, return_probs=True, decision=None, **kw)
    assert np.array_equal(none_map, plain_map) and np.array_equal(none_probs, probs)      # no decision, no change
    assert np.array_equal(infer_tile(inference, raster, decision=None, **kw), infer_tile(inference, raster, **kw))
    q1 = quantise(probs[1])
    differs = False
    for share in (0.25, 0.75):
        decision = Decision.from_q({1: max(1, int(np.quantile(q1, share)))})
        want = decide_host(probs, decision)
        got = infer_tile(inference, raster, decision=decision, **kw)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)       # no probabilities
        got_map, got_probs = infer_tile(inference, raster, return_probs=True, decision=decision, **kw)
        assert np.array_equal(got_map, want) and np.array_equal(got_probs, probs)
        differs |= bool((want != plain_map).any())
        # everything downstream sees the decided map
        config, confident = PatchConfig(8), AttributeConfig(confidence=True)
        st_map, st = infer_tile(inference, raster, decision=decision, stats=True, patches=config, attributes=confident, **kw)
        assert np.array_equal(st_map, want) and np.array_equal(st.counts.reshape(-1), np.bincount(want.reshape(-1), minlength=2))
        _, labels, table = labelled_patches_host(want, 2, config)
        assert st.patches == table and table.n > 0
        assert st.attributes == patch_attributes_host(labels, table, raster, want, probs, AttributeConfig(None, True))
    assert differs
    (key, from_loop), = list(infer_rasters(inference, [("a", raster)], subtile=128, overlap=64, blend="average", device=DEV,
                                           batch_size=4, decision=decision))
    assert key == "a" and np.array_equal(from_loop, want)
