"""Crown-level validation curves on the host (``deadtrees_amd/loss/objects.py``): hand-computed matches, the closure with the
existing chain (``decide_patchwise_host`` -> ``sieve_host`` -> ``overlap_pairs_host`` -> strict IoU), ``ObjectCurves`` and the
argument errors.  Integers throughout: every comparison is exact."""
from fractions import Fraction

import numpy as np
import pytest

import objects_cases as oc
from deadtrees_amd.loss.curves import Decision
from deadtrees_amd.loss.objects import ObjectCurves, ObjectSweep, candidates_host, object_histogram_host

Q = 40000                                # the q of every predicted pixel of the hand cases: jT = jM = 156
J = Q >> 8


def _hand(pred, target, K=2, **sweep):
    """pred / target: small class maps [H, W] -> the curves of one image whose class-c pixels have q_c = Q"""
    pred, target = np.asarray(pred), np.asarray(target)
    q = np.zeros((1, K) + pred.shape, dtype=np.uint16)
    for c in range(1, K):
        q[0, c][pred == c] = Q
    sw = ObjectSweep.from_q({c: 20000 for c in range(1, K)}, **sweep)
    hist, targets, err = object_histogram_host(q, target[None].astype(np.int64), sw)
    assert err == 0 and hist[0].sum() == 0 and targets[0] == 0
    assert hist.sum() == hist[:, :, J, J].sum()                  # every patch lands in the one bin of Q
    return ObjectCurves(hist, targets, sw)


def _at(cv, c, j=J, i=0):
    return tuple(int(v[j]) for v in cv.counts(c, i))


def test_an_iou_of_exactly_one_half_is_no_match_and_one_pixel_more_is():
    target = [[1, 1, 1, 1, 0, 0]]
    half = _hand([[1, 1, 0, 0, 0, 0]], target)                   # n = 2, union = 4
    assert _at(half, 1) == (0, 1, 1)
    more = _hand([[1, 1, 1, 0, 0, 0]], target)                   # n = 3, union = 4
    assert _at(more, 1) == (1, 0, 0)
    assert _at(_hand([[1, 1, 1, 0, 0, 0]], target, min_iou=0.75), 1) == (0, 1, 1)      # exactly 3/4: strict again
    assert _at(_hand([[1, 1, 1, 1, 0, 0]], target, min_iou=0.75), 1) == (1, 0, 0)
    # past the bin of Q nothing is kept: every crown is missed
    assert _at(more, 1, j=J + 1) == (0, 0, 1) and _at(more, 1, i=J + 1) == (0, 0, 1) and _at(more, 1, i=J) == (1, 0, 0)


def test_a_target_without_a_majority_matches_nothing():
    # halved by two predictions of different classes (of one class they would be one patch)
    cv = _hand([[1, 1, 2, 2]], [[1, 1, 1, 1]], K=3)
    assert _at(cv, 1) == (0, 1, 1) and _at(cv, 2) == (0, 1, 0)
    # three thirds: two separate predictions and background
    cv = _hand([[1, 1], [0, 0], [1, 1]], [[1, 1], [1, 1], [1, 1]])
    assert _at(cv, 1) == (0, 2, 1)


def test_one_prediction_over_two_targets():
    assert _at(_hand([[1] * 7], [[1, 1, 1, 0, 1, 1, 1]]), 1) == (0, 1, 2)       # 3 / 7 each
    assert _at(_hand([[1] * 7], [[1, 1, 1, 1, 1, 0, 1]]), 1) == (1, 0, 1)       # 5 / 7 and 1 / 7


def test_classes_must_agree():
    cv = _hand([[1, 1, 1, 0]], [[2, 2, 2, 0]], K=3)
    assert _at(cv, 1) == (0, 1, 0) and _at(cv, 2) == (0, 0, 1)
    assert np.array_equal(cv.targets, [0, 0, 1])


def test_min_pixels_removes_a_matched_prediction():
    pred, target = [[1, 1, 1, 0, 0, 1]], [[1, 1, 1, 0, 0, 0]]
    assert _at(_hand(pred, target), 1) == (1, 1, 0)
    assert _at(_hand(pred, target, min_pixels=2), 1) == (1, 0, 0)               # the single pixel is gone
    assert _at(_hand(pred, target, min_pixels=3), 1) == (1, 0, 0)
    assert _at(_hand(pred, target, min_pixels=4), 1) == (0, 0, 1)               # and now the match: the crown is missed


def test_connectivity_of_both_sides():
    pred, target = [[1, 0], [0, 1]], [[1, 0], [0, 1]]
    assert _at(_hand(pred, target, connectivity=8), 1) == (1, 0, 0)
    assert _at(_hand(pred, target, connectivity=4), 1) == (2, 0, 0)


def test_bad_labels_raise_the_flag_and_are_background():
    q = np.zeros((1, 2, 1, 4), dtype=np.uint16)
    q[0, 1, 0, :3] = Q
    sw = ObjectSweep.from_q({1: 20000})
    clean = object_histogram_host(q, np.array([[[1, 1, 1, 0]]]), sw)
    flagged = object_histogram_host(q, np.array([[[1, 1, 1, 2]]]), sw)
    assert clean[2] == 0 and flagged[2] == 1
    assert np.array_equal(clean[0], flagged[0]) and np.array_equal(clean[1], flagged[1])
    assert object_histogram_host(q, np.array([[[1, 1, 1, -1]]]), sw)[2] == 1


def test_candidates_are_the_pixel_rule_at_the_low_thresholds():
    from deadtrees_amd.loss.curves import decide_host
    rng = np.random.default_rng(0)
    q = (rng.integers(0, 9, (3, 7, 11)) * 8191).astype(np.uint16)                # coarse: ties between the classes
    low = ObjectSweep.from_q({1: 16382, 2: 24573})
    cand, q_own = candidates_host(q, low.low_u16(3))
    assert np.array_equal(cand, decide_host(oc.probs_of(q), Decision.from_q(low.low)))
    assert np.array_equal(q_own, np.where(cand > 0, np.take_along_axis(q.astype(np.int64), cand[None].astype(np.int64), 0)[0], 0))
    assert ((q[1] == q[2]) & (cand == 1)).any()                                 # a real tie went to the smaller class


@pytest.mark.parametrize("min_pixels, min_iou", [(0, 0.5), (4, 0.5), (0, 0.75)])
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("K", [2, 3])
def test_closure_with_the_existing_chain(K, connectivity, min_pixels, min_iou):
    q, target = oc.blobs(oc.CLOSURE_SEEDS[K], 3, K, 19, 33)
    sw = ObjectSweep.from_q(oc.low_for(K), connectivity=connectivity, min_pixels=min_pixels, min_iou=min_iou)
    hist, targets, err = object_histogram_host(q, target, sw)
    cv = ObjectCurves(hist, targets, sw)
    assert err == 0
    rng = np.random.default_rng(100 * K + connectivity)
    for c in range(1, K):
        first = -(-sw.low[c] // 256)
        if (min_pixels, min_iou) == (0, 0.5):                      # never vacuous: a found, an invented and a missed crown
            assert min(_at(cv, c, j=first)) >= 1, (c, _at(cv, c, j=first))
        tp, fp, fn = cv.counts2d(c)
        points = oc.sampled_points(rng, sw.low[c])
        assert len(points) >= 12 and (first, 0) in points
        for j, i in points:
            assert (int(tp[j, i]), int(fp[j, i]), int(fn[j, i])) == oc.chain_counts(q, target, sw, c, j, i), (c, j, i)
    # the operating point read off the curves is the one the chain produces with best_decision() itself
    best = cv.best_decision()
    for c in range(1, K):
        j, i = best.q[c] // 256, best.min_confidence.get(c, 0) // 256
        tp, fp, fn = cv.counts2d(c)
        assert best.q[c] == 256 * j >= sw.low[c]
        assert (int(tp[j, i]), int(fp[j, i]), int(fn[j, i])) == oc.chain_counts(q, target, sw, c, j, i)


def test_the_histogram_adds_over_images():
    q, target = oc.blobs(oc.CLOSURE_SEEDS[3], 3, 3, 19, 33)
    sw = ObjectSweep.from_q(oc.low_for(3))
    whole = object_histogram_host(q, target, sw)
    parts = [object_histogram_host(q[b:b + 1], target[b:b + 1], sw) for b in range(3)]
    assert np.array_equal(whole[0], sum(p[0] for p in parts)) and np.array_equal(whole[1], sum(p[1] for p in parts))


# ---------------------------------------------------------------------- ObjectCurves
def _curves(entries, targets, K=2, low=None):
    """entries: (c, matched, jT, jM, count)"""
    hist = np.zeros((K, 2, 256, 256), dtype=np.int64)
    for c, m, jt, jm, n in entries:
        hist[c, m, jt, jm] += n
    return ObjectCurves(hist, np.asarray(targets, dtype=np.int64), ObjectSweep.from_q(low or {c: 256 for c in range(1, K)}))


def test_object_curves_add_compare_and_are_read_only():
    a = _curves([(1, 1, 200, 100, 3), (1, 0, 50, 20, 2)], [0, 5])
    b = _curves([(1, 1, 200, 100, 1)], [0, 2])
    s = a + b
    assert s.hist[1, 1, 200, 100] == 4 and s.targets[1] == 7 and s == _curves([(1, 1, 200, 100, 4), (1, 0, 50, 20, 2)], [0, 7])
    assert a != b and a == _curves([(1, 1, 200, 100, 3), (1, 0, 50, 20, 2)], [0, 5]) and a.K == 2
    assert "ObjectCurves(K=2, patches=5, targets=5" in repr(a)
    for arr in (a.hist, a.targets):
        with pytest.raises(ValueError):
            arr[...] = 0
    other = ObjectCurves(a.hist, a.targets, ObjectSweep.from_q({1: 256}, connectivity=4))
    assert other != a
    with pytest.raises(ValueError, match="sweeps must be equal"):
        a + other
    with pytest.raises(ValueError, match="hist must be"):
        ObjectCurves(np.zeros((3, 2, 256, 256), np.int64), np.zeros(3, np.int64), ObjectSweep.from_q({1: 256}))
    with pytest.raises(ValueError, match="targets must be"):
        ObjectCurves(np.zeros((2, 2, 256, 256), np.int64), np.zeros(3, np.int64), ObjectSweep.from_q({1: 256}))
    with pytest.raises(ValueError, match="negative"):
        ObjectCurves(np.zeros((2, 2, 256, 256), np.int64), np.array([0, -1]), ObjectSweep.from_q({1: 256}))
    with pytest.raises(ValueError, match="class 0"):
        ObjectCurves(np.zeros((2, 2, 256, 256), np.int64), np.array([1, 0]), ObjectSweep.from_q({1: 256}))
    with pytest.raises(ValueError, match="not in 1..1"):
        a.counts(0)
    with pytest.raises(ValueError, match="confidence index"):
        a.counts(1, 256)


def test_counts_and_average_precision_on_a_hand_histogram():
    # 2 matched patches at jT = 200, 1 unmatched at 150, 1 matched at 100, 4 crowns
    cv = _curves([(1, 1, 200, 90, 2), (1, 0, 150, 60, 1), (1, 1, 100, 30, 1)], [0, 4])
    tp, fp, fn = cv.counts(1)
    assert tp.dtype == np.int64 and tp.shape == (256,)
    assert (tp[:101] == 3).all() and (tp[101:201] == 2).all() and (tp[201:] == 0).all()
    assert (fp[:151] == 1).all() and (fp[151:] == 0).all() and np.array_equal(fn, 4 - tp)
    tp2, fp2, fn2 = cv.counts2d(1)
    assert np.array_equal(tp2[:, 0], tp) and tp2[100, 30] == 3 and tp2[100, 31] == 2 and tp2[0, 91] == 0 and fp2[0, 61] == 0
    assert np.array_equal(cv.counts(1, 61)[1], np.zeros(256, np.int64)) and cv.counts(1, 61)[0][0] == 2
    precision, recall = cv.precision_recall(1)
    assert precision[255] == 1.0 and recall[200] == 0.5 and precision[150] == 2 / 3 and recall[0] == 0.75
    # recall steps: 0 -> 1/2 at j = 200 (precision 1), 1/2 -> 3/4 at j = 100 (precision 3/4)
    assert cv.average_precision(1) == pytest.approx(0.5 * 1.0 + 0.25 * 0.75, abs=1e-15)
    f1 = cv.f1(1)
    assert f1.shape == (256, 256) and f1[100, 0] == pytest.approx(2 * 3 / (2 * 3 + 1 + 1)) and f1[201, 0] == 0.0


def test_best_decision_tie_rules():
    # one matched patch, one crown: F1 = 1 for every j <= 200 and i <= 90 -> the smallest allowed j and i = 0
    cv = _curves([(1, 1, 200, 90, 1)], [0, 1], low={1: 5000})
    d = cv.best_decision()
    assert isinstance(d, Decision) and d == Decision.from_q({1: 256 * 20}, low={1: 5000}) and d.patchwise
    assert cv._best(1) == (20, 0, 1.0)                           # ceil(5000 / 256) = 20
    # an unmatched patch of low confidence: the filter pays, the smallest i that removes it wins, j stays smallest
    cv = _curves([(1, 1, 200, 90, 1), (1, 0, 220, 40, 1)], [0, 1], low={1: 5120})
    d = cv.best_decision()
    assert d.q == {1: 5120} and d.min_confidence == {1: 256 * 41} and d.low == {1: 5120} and d.connectivity == 8
    # where a higher threshold is needed instead: the smallest j that removes the unmatched patch
    cv = _curves([(1, 1, 200, 90, 1), (1, 0, 150, 95, 1)], [0, 1], low={1: 256})
    assert cv.best_decision().q == {1: 256 * 151} and not cv.best_decision().min_confidence
    # K = 3, a class without crowns keeps max(L, 32768); the sweep's connectivity travels
    hist = np.zeros((3, 2, 256, 256), dtype=np.int64)
    hist[1, 1, 200, 90] = 1
    hist[2, 0, 99, 9] = 5
    cv = ObjectCurves(hist, np.array([0, 1, 0]), ObjectSweep.from_q({1: 1000, 2: 40000}, connectivity=4))
    d = cv.best_decision()
    assert d.q == {1: 1024, 2: 40000} and d.low == {1: 1000, 2: 40000} and d.connectivity == 4 and d.K == 3
    cv = ObjectCurves(hist, np.array([0, 1, 0]), ObjectSweep.from_q({1: 1000, 2: 300}))
    assert cv.best_decision().q[2] == 32768


def test_nan_without_targets_and_summary_keys():
    cv = _curves([(1, 0, 99, 9, 5), (2, 1, 200, 90, 2), (2, 0, 220, 40, 1)], [0, 0, 3], K=3)
    assert np.isnan(cv.average_precision(1)) and np.isnan(cv.f1(1)).all() and np.isnan(cv.precision_recall(1)[1]).all()
    s = cv.summary("val")
    assert set(s) == {f"val/crown_{n}_{c}" for c in (1, 2)
                      for n in ("ap", "best_f1", "best_threshold", "best_min_confidence", "targets")}
    assert np.isnan(s["val/crown_ap_1"]) and np.isnan(s["val/crown_best_f1_1"]) and s["val/crown_targets_1"] == 0.0
    assert s["val/crown_best_threshold_1"] == 32768 / 65535 and s["val/crown_best_min_confidence_1"] == 0.0
    assert s["val/crown_best_f1_2"] == pytest.approx(0.8) and s["val/crown_targets_2"] == 3.0
    assert s["val/crown_best_threshold_2"] == 256 / 65535 and s["val/crown_best_min_confidence_2"] == 256 * 41 / 65535
    assert 0.0 <= s["val/crown_ap_2"] <= 1.0
    assert set(cv.summary("test")) == {k.replace("val/", "test/") for k in s}


# ---------------------------------------------------------------------- ObjectSweep
def test_object_sweep_parses_like_a_decision():
    sw = ObjectSweep({1: 0.3, 2: 20000}, connectivity=4, min_pixels=3, min_iou=0.75)
    assert sw.low == {1: 19661, 2: 20000} and sw.K == 3 and (sw.iou_p, sw.iou_q) == (3, 4) and sw.min_iou == Fraction(3, 4)
    assert np.array_equal(sw.low_u16(3), np.array([0, 19661, 20000], dtype=np.uint16)) and sw.low_u16().dtype == np.uint16
    assert sw == ObjectSweep.from_q({2: 20000, 1: 19661}, 4, 3, Fraction(3, 4)) and sw != ObjectSweep.from_q({1: 19661, 2: 20000})
    assert eval(repr(sw)) == sw and hash(sw._key()) == hash(eval(repr(sw))._key())
    assert ObjectSweep({1: 1.0}).low == {1: 65535} and ObjectSweep({1: 1e-9}).low == {1: 1}
    assert (ObjectSweep({1: 0.5}, min_iou=0.6).iou_p, ObjectSweep({1: 0.5}, min_iou=0.6).iou_q) == (3, 5)
    assert len({ObjectSweep.from_q({1: 5}, c, m, i)._key() for c in (4, 8) for m in (0, 2) for i in (0.5, 0.75)}) == 8


@pytest.mark.parametrize("args, kwargs, match", [
    (({},), {}, "non-empty mapping"),
    (([0.5],), {}, "non-empty mapping"),
    (({1: 0.0},), {}, r"ObjectSweep: .*\(0, 1\]"),
    (({1: 1.5},), {}, r"ObjectSweep: .*\(0, 1\]"),
    (({1: float("nan")},), {}, "ObjectSweep: "),
    (({1: 0},), {}, "ObjectSweep: .*1..65535"),
    (({1: 65536},), {}, "ObjectSweep: .*1..65535"),
    (({1: True},), {}, "ObjectSweep: "),
    (({1: "0.5"},), {}, "ObjectSweep: "),
    (({0: 0.5},), {}, "ObjectSweep: class 0"),
    (({8: 0.5},), {}, "ObjectSweep: class 8"),
    (({2: 0.5},), {}, r"ObjectSweep: no low threshold for class\(es\) \[1\]"),
    (({1: 0.5},), {"connectivity": 6}, "ObjectSweep: connectivity"),
    (({1: 0.5},), {"connectivity": True}, "ObjectSweep: connectivity"),
    (({1: 0.5},), {"min_pixels": -1}, "ObjectSweep: min_pixels"),
    (({1: 0.5},), {"min_pixels": 2.0}, "ObjectSweep: min_pixels"),
    (({1: 0.5},), {"min_pixels": True}, "ObjectSweep: min_pixels"),
    (({1: 0.5},), {"min_iou": 0.49}, "ObjectSweep: min_iou"),
    (({1: 0.5},), {"min_iou": 1.0}, "ObjectSweep: min_iou"),
    (({1: 0.5},), {"min_iou": 1 - 1e-9}, "ObjectSweep: min_iou"),
    (({1: 0.5},), {"min_iou": float("nan")}, "ObjectSweep: min_iou"),
    (({1: 0.5},), {"min_iou": "0.5"}, "ObjectSweep: min_iou"),
    (({1: 0.5},), {"min_iou": True}, "ObjectSweep: min_iou"),
])
def test_object_sweep_argument_errors(args, kwargs, match):
    with pytest.raises(ValueError, match=match):
        ObjectSweep(*args, **kwargs)


def test_from_q_and_low_u16_errors():
    with pytest.raises(ValueError, match="ObjectSweep.from_q: .*not an integer"):
        ObjectSweep.from_q({1: 0.5})
    with pytest.raises(ValueError, match="ObjectSweep.from_q: .*not an integer"):
        ObjectSweep.from_q({1: True})
    with pytest.raises(ValueError, match="ObjectSweep: .*K=3"):
        ObjectSweep.from_q({1: 5}).low_u16(3)
    sw = ObjectSweep.from_q({1: 5})
    with pytest.raises(ValueError, match="object_histogram_host: sweep"):
        object_histogram_host(np.zeros((1, 2, 2, 2), np.uint16), np.zeros((1, 2, 2), np.int64), {1: 5})
    with pytest.raises(ValueError, match="object_histogram_host: q must be"):
        object_histogram_host(np.zeros((2, 2, 2), np.uint16), np.zeros((1, 2, 2), np.int64), sw)
    with pytest.raises(ValueError, match="object_histogram_host: q must be"):
        object_histogram_host(np.zeros((1, 2, 2, 2), np.float32), np.zeros((1, 2, 2), np.int64), sw)
    with pytest.raises(ValueError, match="object_histogram_host: target must be"):
        object_histogram_host(np.zeros((1, 2, 2, 2), np.uint16), np.zeros((1, 2, 3), np.int64), sw)
    with pytest.raises(ValueError, match="K=3"):
        object_histogram_host(np.zeros((1, 3, 2, 2), np.uint16), np.zeros((1, 2, 2), np.int64), sw)


def test_check_sweep_names_the_caller():
    from deadtrees_amd.loss.objects import check_sweep, crown_monitors
    sw = ObjectSweep.from_q({1: 5})
    assert check_sweep(None, 2, "validate") is None and check_sweep(sw, 2, "validate") is sw
    with pytest.raises(ValueError, match="validate: objects must be an ObjectSweep"):
        check_sweep(True, 2, "validate")
    with pytest.raises(ValueError, match=r"validate: objects names the classes 1..1, the model has the classes 1..2"):
        check_sweep(sw, 3, "validate")
    assert crown_monitors(3) == ("val/crown_best_f1_1", "val/crown_ap_1", "val/crown_best_f1_2", "val/crown_ap_2")


def test_monitors_accept_crown_scores_only_when_asked():
    from deadtrees_amd.loss.objects import crown_monitors
    from deadtrees_amd.trainer import CheckpointConfig, EarlyStoppingConfig, resolve_checkpoint, resolve_early_stopping
    ck = CheckpointConfig("somewhere", monitor="val/crown_best_f1_1", mode="max")
    es = EarlyStoppingConfig(monitor="val/crown_ap_1", mode="max")
    with pytest.raises(ValueError, match="not a validation metric"):
        resolve_checkpoint(ck, ("GDICE", "FOCAL"))
    with pytest.raises(ValueError, match="not a validation metric"):
        resolve_early_stopping(es, ("GDICE", "FOCAL"))
    assert resolve_checkpoint(ck, ("GDICE", "FOCAL"), extra=crown_monitors(2)).monitor == "val/crown_best_f1_1"
    assert resolve_early_stopping(es, ("GDICE", "FOCAL"), extra=crown_monitors(2)).monitor == "val/crown_ap_1"
    with pytest.raises(ValueError, match="not a validation metric"):
        resolve_checkpoint(CheckpointConfig("somewhere", monitor="val/crown_best_f1_2"), ("GDICE",), extra=crown_monitors(2))
