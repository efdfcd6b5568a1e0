"""``deadtrees_amd/loss/curves.py`` on the CPU: the histogram oracle against a scalar loop, the quantisation, the curve
identities, average precision and ROC AUC against scikit-learn and against a hand-computed case, the best threshold's
ties, ``Decision`` and ``decide_host``, the K = 2 closure between curves and decided maps, and the argument errors of
``validate`` / ``fit`` / ``infer_tile`` that need no device."""
import math

import numpy as np
import pytest

from deadtrees_amd.loss.curves import (BINS, Decision, ProbabilityCurves, check_decision, decide_host, prob_histogram_host,
                                       quantise)


def _q_scalar(p):
    """the quantisation, one value at a time in np.float32 arithmetic"""
    p = np.float32(p)
    p = p if p > 0 else np.float32(0)          # NaN > 0 is False
    p = min(p, np.float32(1))
    return int(math.floor(np.float32(np.float32(p * np.float32(65535)) + np.float32(0.5))))


def _probs(rng, shape, K):
    """fp32 [*shape[:1], K, ...] rows that sum to 1, with a confident background share"""
    p = rng.random((shape[0], K) + tuple(shape[1:])).astype(np.float32) ** 3
    return (p / p.sum(axis=1, keepdims=True)).astype(np.float32)


def test_histogram_oracle_against_a_scalar_loop():
    rng = np.random.default_rng(0)
    B, K, H, W = 1, 3, 5, 7
    p = _probs(rng, (B, H, W), K)
    p[0, 0, 0, 0], p[0, 1, 0, 1], p[0, 2, 0, 2] = np.nan, -0.25, 1.5
    labels = rng.integers(0, K, (B, H, W))
    labels[0, 2, 3] = K                          # outside the range: flagged and skipped
    labels[0, 4, 6] = -1
    lu = rng.integers(0, 3, (B, H, W))
    want = np.zeros((2, K, 2, BINS), dtype=np.int64)
    for y in range(H):
        for x in range(W):
            if 0 <= labels[0, y, x] < K:
                for c in range(K):
                    want[0, c, int(labels[0, y, x] == c), _q_scalar(p[0, c, y, x]) >> 8] += 1
                    want[1, c, int(labels[0, y, x] == c), _q_scalar(p[0, c, y, x]) >> 8] += int(lu[0, y, x] == 1)
    got, err = prob_histogram_host(p, labels, lu)
    assert np.array_equal(got, want) and err == 1 and got.dtype == np.int64
    assert got[0].sum() == K * (H * W - 2) and got[0, 0, :, 0].sum() >= 1 and got[0, 2, :, 255].sum() >= 1
    none, err = prob_histogram_host(p, np.clip(labels, 0, K - 1), None)
    assert err == 0 and none[1].sum() == 0 and none[0].sum() == K * H * W        # no lu: plane 1 is not touched
    # logits mode: a float64 softmax first
    z = rng.normal(0, 4, (2, K, 3, 3)).astype(np.float32)
    lab = rng.integers(0, K, (2, 3, 3))
    e = np.exp(z.astype(np.float64) - z.astype(np.float64).max(1, keepdims=True))
    assert np.array_equal(prob_histogram_host(z, lab, logits=True)[0],
                          prob_histogram_host((e / e.sum(1, keepdims=True)).astype(np.float32), lab)[0])
    with pytest.raises(ValueError):
        prob_histogram_host(p, labels[:, :4], lu)
    with pytest.raises(ValueError):
        prob_histogram_host(p, labels, K=2)


def test_quantisation():
    values = [0.0, 1.0, 127.5 / 65535, 128.4999 / 65535, np.nan, -1.0, 2.0, np.inf, -np.inf]
    got = quantise(np.array(values, dtype=np.float32))
    assert got.tolist() == [_q_scalar(v) for v in values]
    assert got[0] == 0 and got[1] == 65535 and got[4] == 0 and got[5] == 0 and got[6] == 65535 and got[7] == 65535
    assert got[2] == 128 and got[3] == 128                      # 127.5 + 0.5 and 128.4999 + 0.5 both floor to 128
    assert (quantise(np.float32(255.4 / 65535)) >> 8, quantise(np.float32(255.6 / 65535)) >> 8) == (0, 1)


def _curves(seed=1, K=3, n=4000):
    rng = np.random.default_rng(seed)
    p = _probs(rng, (1, n), K)
    labels = np.where(rng.random((1, n)) < 0.7, p.argmax(1), rng.integers(0, K, (1, n)))
    lu = rng.integers(0, 2, (1, n))
    return p, labels, lu, ProbabilityCurves(prob_histogram_host(p, labels, lu)[0])


def test_counts_identities_at_every_threshold():
    p, labels, lu, cv = _curves()
    for masked in (False, True):
        sel = (lu == 1) if masked else np.ones_like(lu, dtype=bool)
        for c in range(cv.K):
            tp, fp, fn, tn = cv.counts(c, masked)
            assert tp.shape == (257,) and tp.dtype == np.int64
            q = quantise(p[:, c])
            P = int(((labels == c) & sel).sum())
            for j in range(257):
                predicted = int(((q >= 256 * j) & sel).sum())
                assert tp[j] + fn[j] == P and tp[j] + fp[j] == predicted
                assert tp[j] + fp[j] + fn[j] + tn[j] == int(sel.sum())
            assert tp[256] == 0 and fp[256] == 0 and tp[0] == P
            precision, recall = cv.precision_recall(c, masked)
            assert precision[256] == 1.0 and recall[256] == 0.0 and recall[0] == 1.0
            f1 = cv.f1(c, masked)
            assert np.allclose(f1[:256], 2 * precision[:256] * recall[:256] / (precision[:256] + recall[:256]), atol=1e-15)


def test_average_precision_and_roc_auc_against_scikit_learn():
    metrics = pytest.importorskip("sklearn.metrics")
    p, labels, lu, cv = _curves(seed=2, K=3, n=6000)
    for masked in (False, True):
        sel = (lu[0] == 1) if masked else np.ones(lu.shape[1], dtype=bool)
        for c in range(3):
            score = (quantise(p[0, c]) >> 8)[sel]
            truth = (labels[0] == c)[sel]
            assert cv.average_precision(c, masked) == pytest.approx(metrics.average_precision_score(truth, score), abs=1e-12)
            assert cv.roc_auc(c, masked) == pytest.approx(metrics.roc_auc_score(truth, score), abs=1e-12)


def test_average_precision_and_roc_auc_by_hand():
    # four pixels, class 1: bins 200 (+), 100 (-), 100 (+), 10 (-)
    hist = np.zeros((2, 2, 2, BINS), dtype=np.int64)
    hist[0, 1, 1, 200] = hist[0, 1, 0, 100] = hist[0, 1, 1, 100] = hist[0, 1, 0, 10] = 1
    cv = ProbabilityCurves(hist)
    # thresholds from above: > 200 nothing; 101..200 (tp 1, fp 0): R 1/2, P 1; 11..100 (tp 2, fp 1): R 1, P 2/3; then (2, 2)
    assert cv.average_precision(1) == pytest.approx(0.5 * 1.0 + 0.5 * (2 / 3), abs=1e-15)
    # ROC points (fpr, tpr): (0, 0), (0, 1/2), (1/2, 1), (1, 1): area 0 + 1/2 * 3/4 + 1/2 * 1
    assert cv.roc_auc(1) == pytest.approx(0.875, abs=1e-15)
    tp, fp, fn, tn = cv.counts(1)
    assert (tp[201], tp[200], tp[101], tp[100], tp[11], tp[10]) == (0, 1, 1, 2, 2, 2)
    assert (fp[101], fp[100], fp[11], fp[10], fp[0]) == (0, 1, 1, 2, 2)
    assert cv.best_threshold(1) == (256 * 11, 0.8)               # F1 = 4 / 5 on j in 11..100: ties go to the smallest j
    assert cv.best_threshold(1, "recall_at_precision", 0.9) == (256 * 101, 0.5)
    assert cv.best_threshold(1, "precision_at_recall", 0.9) == (256 * 11, pytest.approx(2 / 3))
    assert cv.best_threshold(1, "precision_at_recall", 0.5) == (256 * 101, 1.0)
    count, positives, centre = cv.reliability(1)
    assert count.sum() == 4 and positives.sum() == 2 and centre[0] == 127.5 / 65535 and centre[255] == (65280 + 127.5) / 65535
    want = (abs(1 - centre[200]) + 2 * abs(0.5 - centre[100]) + abs(0 - centre[10])) / 4
    assert cv.ece(1) == pytest.approx(want, abs=1e-15)
    assert math.isnan(cv.ece(1, masked=True))


def test_a_class_without_positives_gives_nan_and_bad_arguments_raise():
    hist = np.zeros((2, 3, 2, BINS), dtype=np.int64)
    hist[0, :, 0, 3] = 5                                         # five pixels, all of class ... none: no positives anywhere
    hist[0, 0, 1, 250], hist[0, 0, 0, 3] = 5, 0                  # class 0 has them all
    cv = ProbabilityCurves(hist, ["background", "dead", "other"])
    for c in (1, 2):
        assert math.isnan(cv.average_precision(c)) and math.isnan(cv.roc_auc(c)) and np.isnan(cv.f1(c)).all()
        T, score = cv.best_threshold(c)
        assert T is None and math.isnan(score)
        assert cv.best_threshold(c, "recall_at_precision", 0.5)[0] is None
    assert math.isnan(cv.roc_auc(0))                             # no negatives
    s = cv.summary("val")
    assert sorted(s) == sorted(f"val/{k}_{c}" for c in (1, 2) for k in ("ap", "roc_auc", "best_f1", "best_threshold"))
    assert all(isinstance(v, float) and math.isnan(v) for v in s.values())
    assert "array" not in repr(cv) and "dead" in repr(cv) and "pixels=5" in repr(cv)
    with pytest.raises(ValueError):
        cv.counts(3)
    with pytest.raises(ValueError):
        cv.best_threshold(1, "accuracy")
    with pytest.raises(ValueError):
        cv.best_threshold(1, "recall_at_precision")
    with pytest.raises(ValueError):
        cv.best_threshold(1, "f1", 0.5)
    with pytest.raises(ValueError):
        ProbabilityCurves(np.zeros((2, 3, 2, 255), dtype=np.int64))
    with pytest.raises(ValueError):
        ProbabilityCurves(hist, ["a", "b"])
    with pytest.raises(ValueError):
        ProbabilityCurves(-hist)


def test_curves_add_and_compare():
    rng = np.random.default_rng(3)
    p, labels = _probs(rng, (2, 500), 2), rng.integers(0, 2, (2, 500))
    lu = rng.integers(0, 2, (2, 500))
    whole = ProbabilityCurves(prob_histogram_host(p, labels, lu)[0])
    parts = [ProbabilityCurves(prob_histogram_host(p[i:i + 1], labels[i:i + 1], lu[i:i + 1])[0]) for i in range(2)]
    assert parts[0] + parts[1] == whole and parts[0] != whole and (parts[0] + parts[1]).hist.dtype == np.int64
    assert whole.summary() == (parts[1] + parts[0]).summary()
    with pytest.raises(ValueError):
        whole + ProbabilityCurves(np.zeros((2, 3, 2, BINS), dtype=np.int64))
    with pytest.raises(TypeError):
        whole + 1


def test_decision_conversion_and_errors():
    d = Decision({1: 0.5, 2: 1.0, 3: 1e-9})
    assert d.q == {1: 32768, 2: 65535, 3: 1} and d.K == 4        # floor(32767.5 + 0.5); clipped to 1 from below
    assert d.thresholds_u16().tolist() == [0, 32768, 65535, 1] and d.thresholds_u16().dtype == np.uint16
    assert Decision({1: 300}).q == {1: 300} and Decision.from_q({1: 256 * 77}) == Decision({1: 19712})
    assert Decision({1: np.float32(0.25)}).q == {1: int(math.floor(0.25 * 65535 + 0.5))}
    assert repr(Decision({1: 0.5})) == "Decision.from_q({1: 32768})"
    for bad in ({}, {1: 0.0}, {1: 1.5}, {1: float("nan")}, {1: 0}, {1: 65536}, {1: True}, {1: "0.5"}, {0: 0.5}, {8: 0.5},
                {2: 0.5}, {1: 0.5, 3: 0.5}, [0.5], None, {1.0: 0.5}):
        with pytest.raises(ValueError):
            Decision(bad)
    with pytest.raises(ValueError):
        Decision.from_q({1: 0.5})
    with pytest.raises(ValueError):
        d.thresholds_u16(3)                                      # a class too many
    with pytest.raises(ValueError, match="infer_tile"):
        check_decision(Decision({1: 0.5}), 3, "infer_tile")      # class 2 is missing
    with pytest.raises(ValueError, match="infer_tile"):
        check_decision({1: 0.5}, 2, "infer_tile")
    assert check_decision(None, 2, "infer_tile") is None and check_decision(d, 4, "infer_tile") is d


def test_decide_host_rule_and_ties():
    one = np.float32(1.0)
    T = {1: 256 * 100, 2: 256 * 50}
    # columns: nobody reaches; only 2 reaches; both reach, 1 larger; both reach, equal q (tie -> 1); 2 larger; NaN and > 1
    p1 = np.array([0.2, 0.1, 0.6, 0.5, 0.45, np.nan], dtype=np.float32)
    p2 = np.array([0.1, 0.3, 0.4, 0.5, 0.55, 1.5], dtype=np.float32)
    probs = np.stack([one - p1 - p2, p1, p2]).astype(np.float32)
    got = decide_host(probs, Decision.from_q(T))
    assert got.dtype == np.uint8 and got.tolist() == [0, 2, 1, 1, 2, 2]
    # class 0's probability is never read: a background of 0.9 does not stop a candidate
    probs[0] = 0.9
    assert decide_host(probs, Decision.from_q(T)).tolist() == [0, 2, 1, 1, 2, 2]
    # exactly at the threshold is a candidate; one q below is not
    edge = np.array([[0.5, 0.5], [25600 / 65535, 25599 / 65535], [0, 0]], dtype=np.float32)
    assert quantise(edge[1]).tolist() == [25600, 25599] and decide_host(edge, Decision.from_q(T)).tolist() == [1, 0]
    assert decide_host(np.zeros((3, 4, 5), dtype=np.float32), Decision.from_q(T)).shape == (4, 5)
    with pytest.raises(ValueError):
        decide_host(probs, Decision({1: 0.5}))


@pytest.mark.parametrize("j", [1, 77, 128, 255])
def test_k2_closure_between_curves_and_decided_maps(j):
    rng = np.random.default_rng(5)
    p = _probs(rng, (3, 40, 50), 2)
    labels, lu = rng.integers(0, 2, (3, 40, 50)), rng.integers(0, 2, (3, 40, 50))
    cv = ProbabilityCurves(prob_histogram_host(p, labels, lu)[0])
    decided = np.stack([decide_host(p[b], Decision.from_q({1: 256 * j})) for b in range(3)])
    for masked in (False, True):
        sel = (lu == 1) if masked else np.ones(lu.shape, dtype=bool)
        tp, fp, fn, tn = (int(v[j]) for v in cv.counts(1, masked))
        assert tp == int(((decided == 1) & (labels == 1) & sel).sum()) and fp == int(((decided == 1) & (labels == 0) & sel).sum())
        assert fn == int(((decided == 0) & (labels == 1) & sel).sum()) and tn == int(((decided == 0) & (labels == 0) & sel).sum())
    assert 0 < tp + fp < p.shape[0] * 40 * 50 or j in (1, 255)


class _Inference:
    classes = 2

    def run_windows(self, *a, **k):
        raise AssertionError("nothing may run before the arguments are checked")


def test_argument_errors_that_need_no_device():
    from deadtrees_amd.deployment.tiler import infer_rasters, infer_tile
    from deadtrees_amd.trainer import HipTrainer, fit
    raster = np.zeros((3, 64, 64), dtype=np.uint8)
    d = Decision({1: 0.3})
    with pytest.raises(ValueError, match="infer_tile.*overlap"):
        infer_tile(_Inference(), raster, decision=d)                                    # the block path has no probabilities
    with pytest.raises(ValueError, match="infer_tile.*average"):
        infer_tile(_Inference(), raster, overlap=16, blend="crop", decision=d)
    with pytest.raises(ValueError, match="infer_tile"):
        infer_tile(_Inference(), raster, overlap=16, blend="average", decision={1: 0.3})
    with pytest.raises(ValueError, match="infer_tile"):
        infer_tile(_Inference(), raster, overlap=16, blend="average", decision=Decision({1: 0.3, 2: 0.3}))
    with pytest.raises(ValueError, match="infer_rasters"):
        next(infer_rasters(_Inference(), [raster], decision=d))

    class Ensemble(_Inference):
        members, vote = [_Inference(), _Inference()], "hard"
    with pytest.raises(ValueError, match="soft"):
        infer_tile(Ensemble(), raster, overlap=16, blend="average", decision=d)
    with pytest.raises(ValueError, match="curves"):
        HipTrainer.validate(object.__new__(HipTrainer), [], curves="yes")
    with pytest.raises(ValueError, match="curves"):
        fit(None, [], 1, curves=True)                                                   # no val_loader
    with pytest.raises(ValueError, match="curves"):
        fit(None, [], 1, val_loader=[], curves=1)
