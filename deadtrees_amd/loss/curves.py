"""Operating points: what every threshold on a class probability would cost, and the decision that applies one.

Every map of this project is an arg-max map; on a rare class (dead trees: about 3 % cover) the arg-max is seldom the
operating point a forester wants.  A validation epoch therefore collects, per class, a histogram of the predicted
probability split by ground truth (``ProbabilityCurves``: precision / recall, ROC, F1, calibration, the best threshold),
and inference can decide its maps at such a threshold (``Decision``) before every downstream analysis.

The contract, in one place (the device path, ``csrc/curves.hip`` through ``ops.prob_histogram`` and
``ops.decide_classes``, computes exactly this; ``prob_histogram_host`` and ``decide_host`` are the CPU path).  Everything is
an integer, so device and host compare with ``array_equal``:

* quantisation — the rule of ``deployment/attributes.py``'s confidence, imported from there: ``p' = p if p > 0 else 0`` (NaN
  becomes 0), ``p' = min(p', 1)`` and ``q = floor(p' * 65535 + 0.5)``, the product and the sum each rounded to float32
  (``np.float32`` arithmetic here, ``-ffp-contract=off`` and ``__fmul_rn`` / ``__fadd_rn`` there).  ``q`` lies in
  ``[0, 65535]`` and ``bin = q >> 8``: 256 bins;
* ``hist`` is int64 ``[2, K, 2, 256]``, indexed ``[plane, c, t, bin]``, ``2 <= K <= 8``.  Plane 0 counts every pixel, plane 1
  the pixels with ``lu == 1`` (no ``lu``: plane 1 stays as it was, the rule of ``dt_confusion_matrix``).  ``c`` is the class
  whose probability is binned — every pixel adds K entries per plane — and ``t = 1`` iff ``label == c``.  A label outside
  ``[0, K)`` raises the int32 error flag and the pixel enters no count.  Histograms add across batches, ranks and rasters;
* threshold index ``j`` in ``0..256`` means "predict ``c`` iff ``q_c >= 256 j``": ``tp[j] = sum(hist[plane, c, 1, j:])``, and
  ``j = 256`` predicts nothing;
* decision: thresholds ``T_c`` in ``1..65535`` for every class ``c >= 1``.  The candidates of a pixel are the classes
  ``c >= 1`` with ``q_c >= T_c``; without a candidate the pixel is class 0, otherwise it takes the candidate with the largest
  ``q_c``, ties to the smallest ``c``.  For K = 2 this is "class 1 iff ``q_1 >= T_1``": whenever ``T_1`` is a multiple of 256,
  the confusion counts of the decided maps ARE ``counts(1)`` at ``j = T_1 / 256``, bit for bit.  For K > 2 the curves are
  one-vs-rest and the decision is the rule above: the closure is exact for K = 2 only;
* patch-wise decision (``ops.decide_patchwise`` on the device, ``decide_patchwise_host`` here): a hysteresis
  with low thresholds ``1 <= L_c <= T_c`` and a confidence filter ``M_c`` in ``0..65535`` (0: none), for ``probs`` fp32
  ``[K, h, w]``, sides ``<= 16384``, ``h * w <= 2**31 - 2``, ``2 <= K <= 8``:

  1. ``cand = decide_host(probs, Decision.from_q(L))`` — the pixel rule above at the low thresholds;
  2. ``labels = label_patches_host(cand, K, connectivity)`` — the label plane of ``deployment/patches.py``;
  3. per patch ``P`` of class ``c``, with ``q(p) = quantise(probs[c, p])``: ``qmax = max q``, ``S = sum q`` (int64),
     ``A = |P|``; ``P`` is kept iff ``qmax >= T_c`` and ``S >= M_c * A``, a 64-bit integer compare;
  4. the result is ``cand`` on kept patches and 0 elsewhere.

  With ``L = T`` and no ``M`` this is ``decide_host(probs, Decision(T))`` (every candidate is its own proof).  For K = 2
  and no ``M``, pixel by pixel: decided at ``T`` ⊆ result ⊆ decided at ``L``.  For K > 2 only the rule itself holds — a pixel
  that is class 1 at ``T`` can be a class-2 candidate at ``L`` (``q_2 >= L_2`` and ``q_2 > q_1``), as the curves above are
  one-vs-rest.  Relabelling the result with the same connectivity gives exactly the kept patches of ``cand``, with their
  roots: a patch goes or stays whole, and two kept patches of one class never touch.  Object-level precision / recall
  sweeps over ``(T, M)`` at one ``L`` are ``loss/objects.py``.  Out of scope: sweeps over ``L`` inside one
  pass, the ``against`` map, decisions stored in checkpoints, temperature scaling.

Validation probabilities are single-tile softmaxes and raster probabilities are blended ones (``infer_tile`` with
``blend="average"``): a threshold transfers, but the exact closure is a statement about identical inputs.

numpy and the standard library only (the patch-wise host rule labels with ``label_patches_host``, which imports scipy lazily).
"""
from __future__ import annotations

import math
from typing import Mapping, Optional, Sequence, Tuple

import numpy as np

from ..deployment.attributes import Q_SCALE, confidence_q

BINS = 256
MAX_CLASSES = 8
METRICS = ("f1", "recall_at_precision", "precision_at_recall")


def quantise(p) -> np.ndarray:
    """int64: ``q`` of the contract, elementwise over float32 values (``attributes.confidence_q``)"""
    return confidence_q(p)


def _softmax64(z: np.ndarray) -> np.ndarray:
    z = z.astype(np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def prob_histogram_host(src, labels, lu=None, K: Optional[int] = None, logits: bool = False):
    """the numpy oracle of ``ops.prob_histogram``: ``src`` ``[B, K, ...]`` probabilities (``logits=True``: logits, through a
    float64 softmax first), ``labels`` and ``lu`` ``[B, ...]`` -> ``(hist int64 [2, K, 2, 256], err)``; ``err`` is 1 when a
    label lies outside ``[0, K)``"""
    src = np.asarray(src)
    if src.ndim < 2:
        raise ValueError(f"prob_histogram_host: src must be [B, K, ...], got shape {src.shape}")
    B, k = src.shape[0], src.shape[1]
    K = k if K is None else int(K)
    if K != k or not 2 <= K <= MAX_CLASSES:
        raise ValueError(f"prob_histogram_host: {k} class planes for K={K} (2..{MAX_CLASSES})")
    src = src.reshape(B, K, -1)
    return q_histogram_host(quantise(_softmax64(src) if logits else src), labels, lu)


def q_histogram_host(q, labels, lu=None):
    """``prob_histogram_host`` behind the quantisation: ``q`` integers ``[B, K, ...]`` in ``0..65535`` (what
    ``ops.prob_histogram(..., want_q=True)`` hands back) -> ``(hist, err)``"""
    q = np.asarray(q)
    B, K = q.shape[0], q.shape[1]
    if not 2 <= K <= MAX_CLASSES:
        raise ValueError(f"q_histogram_host: K={K} (2..{MAX_CLASSES})")
    bins = q.reshape(B, K, -1).astype(np.int64) >> 8
    labels = np.asarray(labels).reshape(B, -1).astype(np.int64)
    if labels.shape[1] != bins.shape[2]:
        raise ValueError("prob_histogram_host: src and labels must have the same number of pixels")
    valid = (labels >= 0) & (labels < K)
    planes = [valid]
    if lu is not None:
        lu = np.asarray(lu).reshape(B, -1)
        if lu.shape != labels.shape:
            raise ValueError("prob_histogram_host: lu and labels must have the same number of pixels")
        planes.append(valid & (lu == 1))
    hist = np.zeros((2, K, 2, BINS), dtype=np.int64)
    for plane, sel in enumerate(planes):
        for c in range(K):
            for t in (0, 1):
                here = sel & ((labels == c) == bool(t))
                hist[plane, c, t] = np.bincount(bins[:, c][here], minlength=BINS)
    return hist, int(not valid.all())


class ProbabilityCurves:
    """the curves of one histogram ``[2, K, 2, 256]``.  ``masked=True`` reads plane 1 (``lu == 1``).  Arrays over the
    threshold index have 257 entries (``j = 0`` predicts ``c`` everywhere, ``j = 256`` nowhere); a class without positives
    gives ``nan``, never an exception.  ``+`` adds the histograms of two epochs, ranks or rasters."""

    def __init__(self, hist, class_names: Optional[Sequence[str]] = None):
        hist = np.asarray(hist)
        if hist.ndim != 4 or hist.shape[0] != 2 or hist.shape[2] != 2 or hist.shape[3] != BINS \
                or not 2 <= hist.shape[1] <= MAX_CLASSES:
            raise ValueError(f"ProbabilityCurves: hist must be [2, K, 2, {BINS}] with K in 2..{MAX_CLASSES}, got {hist.shape}")
        if not np.issubdtype(hist.dtype, np.integer) and not np.array_equal(hist, np.floor(hist)):
            raise ValueError("ProbabilityCurves: counts are integers")
        self.hist = hist.astype(np.int64)
        if (self.hist < 0).any():
            raise ValueError("ProbabilityCurves: counts must not be negative")
        self.K = int(hist.shape[1])
        if class_names is not None:
            class_names = tuple(str(n) for n in class_names)
            if len(class_names) != self.K:
                raise ValueError(f"ProbabilityCurves: {len(class_names)} class names for K={self.K}")
        self.class_names = class_names

    def __add__(self, other):
        if not isinstance(other, ProbabilityCurves):
            return NotImplemented
        if other.K != self.K:
            raise ValueError(f"ProbabilityCurves: K={self.K} + K={other.K}")
        return ProbabilityCurves(self.hist + other.hist, self.class_names if self.class_names is not None else other.class_names)

    def __eq__(self, other) -> bool:
        if not isinstance(other, ProbabilityCurves):
            return NotImplemented
        return self.K == other.K and np.array_equal(self.hist, other.hist)

    __hash__ = None

    def __repr__(self) -> str:
        names = "" if self.class_names is None else f", classes={list(self.class_names)}"
        return (f"ProbabilityCurves(K={self.K}, pixels={int(self.hist[0, 0].sum())}, "
                f"masked_pixels={int(self.hist[1, 0].sum())}{names})")

    def _class(self, c) -> int:
        if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= c < self.K:
            raise ValueError(f"ProbabilityCurves: class {c!r} is not in 0..{self.K - 1}")
        return int(c)

    # ------------------------------------------------------------------ counts per threshold index
    def counts(self, c: int, masked: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """``(tp, fp, fn, tn)`` int64 [257] of "predict ``c`` iff ``q_c >= 256 j``" """
        h = self.hist[1 if masked else 0, self._class(c)]
        tp = np.concatenate([np.cumsum(h[1, ::-1])[::-1], [0]]).astype(np.int64)
        fp = np.concatenate([np.cumsum(h[0, ::-1])[::-1], [0]]).astype(np.int64)
        return tp, fp, tp[0] - tp, fp[0] - fp

    def precision_recall(self, c: int, masked: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """``(precision, recall)`` fp64 [257]; precision is 1.0 where nothing is predicted, recall ``nan`` without positives"""
        tp, fp, fn, _ = self.counts(c, masked)
        pred, pos = tp + fp, int(tp[0])
        precision = np.where(pred > 0, tp / np.maximum(pred, 1), 1.0)
        recall = tp / pos if pos > 0 else np.full(tp.shape, np.nan)
        return precision, recall

    def average_precision(self, c: int, masked: bool = False) -> float:
        """the step sum ``sum_j (R_j - R_{j+1}) * P_j``: scikit-learn's ``average_precision_score`` with the bin index as score"""
        precision, recall = self.precision_recall(c, masked)
        return float(np.sum((recall[:-1] - recall[1:]) * precision[:-1]))

    def roc(self, c: int, masked: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """``(fpr, tpr)`` fp64 [257], from (1, 1) at ``j = 0`` down to (0, 0); ``nan`` without negatives / positives"""
        tp, fp, _, _ = self.counts(c, masked)
        pos, neg = int(tp[0]), int(fp[0])
        nan = np.full(tp.shape, np.nan)
        return (fp / neg if neg > 0 else nan), (tp / pos if pos > 0 else nan)

    def roc_auc(self, c: int, masked: bool = False) -> float:
        """the trapezoid under ``roc``: scikit-learn's ``roc_auc_score`` with the bin index as score"""
        fpr, tpr = self.roc(c, masked)
        return float(np.sum((fpr[:-1] - fpr[1:]) * (tpr[:-1] + tpr[1:]) * 0.5))

    def f1(self, c: int, masked: bool = False) -> np.ndarray:
        """fp64 [257]: ``2 tp / (2 tp + fp + fn)``"""
        tp, fp, fn, _ = self.counts(c, masked)
        if int(tp[0]) == 0:
            return np.full(tp.shape, np.nan)
        return 2.0 * tp / (2 * tp + fp + fn)

    def best_threshold(self, c: int, metric: str = "f1", value: Optional[float] = None, masked: bool = False):
        """``(T, score)`` with ``T = 256 j``, ``1 <= j <= 255``, ties to the smallest ``j``.  ``"f1"``: the largest F1;
        ``"recall_at_precision"``: the largest recall among the thresholds whose precision is at least ``value``;
        ``"precision_at_recall"``: the largest precision among those whose recall is at least ``value``.  ``(None, nan)`` for
        a class without positives, or where no threshold meets ``value``"""
        if metric not in METRICS:
            raise ValueError(f"best_threshold: metric {metric!r}: use one of {METRICS}")
        if metric == "f1":
            if value is not None:
                raise ValueError("best_threshold: metric 'f1' takes no value")
            score, allowed = self.f1(c, masked), None
        else:
            if value is None or isinstance(value, bool) or not 0.0 <= float(value) <= 1.0:
                raise ValueError(f"best_threshold: metric {metric!r} needs a value in [0, 1], got {value!r}")
            precision, recall = self.precision_recall(c, masked)
            score, bound = (recall, precision) if metric == "recall_at_precision" else (precision, recall)
            allowed = bound >= float(value)                      # (nan compares False)
        score = score[1:BINS].copy()
        if allowed is not None:
            score[~allowed[1:BINS]] = np.nan
        if np.isnan(score).all():
            return None, float("nan")
        j = int(np.nanargmax(score)) + 1                         # the first of equal maxima
        return BINS * j, float(score[j - 1])

    # ------------------------------------------------------------------ calibration
    def reliability(self, c: int, masked: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """per bin ``(count int64 [256], positives int64 [256], centre fp64 [256])``, centre ``(256 b + 127.5) / 65535``"""
        h = self.hist[1 if masked else 0, self._class(c)]
        return h[0] + h[1], h[1].copy(), (BINS * np.arange(BINS) + 127.5) / Q_SCALE

    def ece(self, c: int, masked: bool = False) -> float:
        """expected calibration error over the 256 bins: ``sum_b count_b / n * |positives_b / count_b - centre_b|``"""
        count, positives, centre = self.reliability(c, masked)
        n = int(count.sum())
        if n == 0:
            return float("nan")
        used = count > 0
        return float(np.sum(count[used] / n * np.abs(positives[used] / count[used] - centre[used])))

    def summary(self, prefix: str = "val") -> dict:
        """the scalars ``fit`` logs, for every class ``c >= 1``: ``{prefix}/ap_<c>``, ``/roc_auc_<c>``, ``/best_f1_<c>`` and
        ``/best_threshold_<c>`` (the float ``T / 65535``; ``nan`` without positives)"""
        out = {}
        for c in range(1, self.K):
            T, best = self.best_threshold(c)
            out[f"{prefix}/ap_{c}"] = self.average_precision(c)
            out[f"{prefix}/roc_auc_{c}"] = self.roc_auc(c)
            out[f"{prefix}/best_f1_{c}"] = best
            out[f"{prefix}/best_threshold_{c}"] = float("nan") if T is None else T / Q_SCALE
        return out


def _threshold(c, t) -> int:
    if isinstance(t, (bool, np.bool_)):
        raise ValueError(f"Decision: threshold {t!r} of class {c}: a float in (0, 1] or an int in 1..{Q_SCALE}")
    if isinstance(t, (int, np.integer)):
        if not 1 <= t <= Q_SCALE:
            raise ValueError(f"Decision: threshold {t!r} of class {c}: an int is a q in 1..{Q_SCALE}")
        return int(t)
    if isinstance(t, (float, np.floating)):
        if not 0.0 < float(t) <= 1.0:                              # (nan fails too)
            raise ValueError(f"Decision: threshold {t!r} of class {c}: a float is a probability in (0, 1]")
        return min(max(int(math.floor(float(t) * Q_SCALE + 0.5)), 1), Q_SCALE)
    raise ValueError(f"Decision: threshold {t!r} of class {c}: a float in (0, 1] or an int in 1..{Q_SCALE}")


def _class_thresholds(thresholds, what: str) -> dict:
    """a mapping class -> threshold, parsed by ``_threshold``: ``{c: q}`` in ascending ``c``"""
    if not isinstance(thresholds, Mapping):
        raise ValueError(f"Decision: {what} must be a mapping class -> threshold, got {thresholds!r}")
    q = {}
    for c, t in thresholds.items():
        if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 1 <= c < MAX_CLASSES:
            raise ValueError(f"Decision: class {c!r} is not in 1..{MAX_CLASSES - 1}")
        q[int(c)] = _threshold(c, t)
    return {c: q[c] for c in sorted(q)}


class Decision:
    """a threshold per class ``1..K-1``: ``Decision({1: 0.3})`` for K = 2, ``Decision({1: 0.3, 2: 0.5})`` for K = 3.  A float in
    ``(0, 1]`` becomes ``T = floor(t * 65535 + 0.5)`` (float64, clipped to ``[1, 65535]``), an int is taken as ``T``
    (``Decision.from_q`` takes integers only).  Every class from 1 to the largest one named must be there; ``K`` is that
    largest class + 1 and must be the model's.  The rule is the module's contract.

    Patch-wise (``decide_patchwise_host`` states the rule): ``low`` names a low threshold ``L_c <= T_c`` for exactly the
    classes of ``thresholds`` (None: ``L = T``), ``min_confidence`` a minimum mean ``M_c`` of a patch's quantised probability
    for any of them (absent: 0, no filter), both parsed like ``thresholds``; ``connectivity`` (4 or 8) is that of the
    candidates' patches.  ``patchwise`` tells whether any of this changes a map: a decision with ``L = T`` and no ``M`` IS
    the plain decision — it compares equal to it, prints like it and takes its code path."""

    def __init__(self, thresholds: Mapping[int, float], low: Optional[Mapping[int, float]] = None,
                 min_confidence: Optional[Mapping[int, float]] = None, connectivity: int = 8):
        if not isinstance(thresholds, Mapping) or not thresholds:
            raise ValueError(f"Decision: a non-empty mapping class -> threshold, got {thresholds!r}")
        q = _class_thresholds(thresholds, "thresholds")
        missing = sorted(set(range(1, max(q) + 1)) - set(q))
        if missing:
            raise ValueError(f"Decision: no threshold for class(es) {missing}: every class 1..K-1 must be named")
        self.q = q
        if isinstance(connectivity, (bool, np.bool_)) or connectivity not in (4, 8):
            raise ValueError(f"Decision: connectivity must be 4 or 8, got {connectivity!r}")
        self.connectivity = int(connectivity)
        self.low = dict(q)
        if low is not None:
            self.low = _class_thresholds(low, "low")
            if set(self.low) != set(q):
                raise ValueError(f"Decision: low names the classes {sorted(self.low)}, thresholds the classes {sorted(q)}: "
                                 "they must be the same")
            above = [c for c in q if self.low[c] > q[c]]
            if above:
                raise ValueError(f"Decision: low threshold above the high one for class(es) {above}: "
                                 f"low {self.low}, thresholds {q} (on the q axis)")
        self.min_confidence = {}
        if min_confidence is not None:
            self.min_confidence = _class_thresholds(min_confidence, "min_confidence")
            unknown = sorted(set(self.min_confidence) - set(q))
            if unknown:
                raise ValueError(f"Decision: min_confidence names class(es) {unknown} that thresholds does not")

    @classmethod
    def from_q(cls, thresholds: Mapping[int, int], low: Optional[Mapping[int, int]] = None,
               min_confidence: Optional[Mapping[int, int]] = None, connectivity: int = 8) -> "Decision":
        """thresholds given as integers ``T`` (``L``, ``M``) on the ``q`` axis, taken as they are"""
        for given in (thresholds, low, min_confidence):
            if isinstance(given, Mapping):
                for c, t in given.items():
                    if isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, np.integer)):
                        raise ValueError(f"Decision.from_q: threshold {t!r} of class {c!r} is not an integer")
        return cls(thresholds, low=low, min_confidence=min_confidence, connectivity=connectivity)

    @property
    def K(self) -> int:
        return len(self.q) + 1

    @property
    def patchwise(self) -> bool:
        """True iff some ``L_c < T_c`` or some ``M_c > 0``: the decision looks at patches, not at pixels alone"""
        return self.low != self.q or bool(self.min_confidence)

    def _u16(self, values: Mapping[int, int], K: Optional[int]) -> np.ndarray:
        if K is not None and int(K) != self.K:
            raise ValueError(f"Decision: thresholds for the classes 1..{self.K - 1}, but K={K}: every class 1..K-1 must be "
                             "named, and no other")
        return np.array([0] + [values.get(c, 0) for c in range(1, self.K)], dtype=np.uint16)

    def thresholds_u16(self, K: Optional[int] = None) -> np.ndarray:
        """uint16 [K]: ``T_c`` at index ``c``, 0 (not read) at index 0; a ``K`` other than this decision's is a ``ValueError``"""
        return self._u16(self.q, K)

    def low_u16(self, K: Optional[int] = None) -> np.ndarray:
        """uint16 [K]: ``L_c`` at index ``c`` (``T_c`` without ``low``), 0 at index 0"""
        return self._u16(self.low, K)

    def min_confidence_u16(self, K: Optional[int] = None) -> np.ndarray:
        """uint16 [K]: ``M_c`` at index ``c``, 0 for a class without a filter and at index 0"""
        return self._u16(self.min_confidence, K)

    def _key(self):
        if not self.patchwise:                                     # the connectivity of a pixel rule changes no map
            return (self.q,)
        return self.q, self.low, self.min_confidence, self.connectivity

    def __eq__(self, other) -> bool:
        if not isinstance(other, Decision):
            return NotImplemented
        return self._key() == other._key()

    __hash__ = None

    def __repr__(self) -> str:
        if not self.patchwise:
            return f"Decision.from_q({self.q!r})"
        low = f", low={self.low!r}" if self.low != self.q else ""
        conf = f", min_confidence={self.min_confidence!r}" if self.min_confidence else ""
        return f"Decision.from_q({self.q!r}{low}{conf}, connectivity={self.connectivity})"


def check_decision(option, K: Optional[int], caller: str) -> Optional[Decision]:
    """the ``decision`` argument of ``infer_tile`` / ``infer_rasters`` -> ``Decision`` or None; a wrong type, a class outside
    ``1..K-1`` or a missing class is a ``ValueError`` naming the caller"""
    if option is None:
        return None
    if not isinstance(option, Decision):
        raise ValueError(f"{caller}: decision must be a Decision or None, got {option!r}")
    if K is not None and option.K != int(K):
        raise ValueError(f"{caller}: decision names the classes 1..{option.K - 1}, the model has the classes 1..{int(K) - 1}")
    return option


def decide_host(probs, decision: Decision) -> np.ndarray:
    """the numpy form of ``ops.decide_classes``: fp32 ``[K, ...]`` probabilities -> uint8 ``[...]`` class map"""
    probs = np.asarray(probs, dtype=np.float32)
    if probs.ndim < 2:
        raise ValueError(f"decide_host: probs must be [K, ...], got shape {probs.shape}")
    T = decision.thresholds_u16(probs.shape[0]).astype(np.int64)
    q = quantise(probs[1:])
    q = np.where(q >= T[1:].reshape((-1,) + (1,) * (probs.ndim - 1)), q, -1)
    best = np.argmax(q, axis=0)                                   # the first of equal maxima: the smallest class
    return np.where(np.take_along_axis(q, best[None], 0)[0] >= 0, best + 1, 0).astype(np.uint8)


# ---------------------------------------------------------------------- patch-wise decisions
MAX_SIDE = 16384
MAX_PIXELS = 2 ** 31 - 2      # labels are int32 and 1-based (``deployment/patches.py``)


def _check_plane_shape(shape, what: str) -> None:
    if len(shape) != 2 or min(shape) < 1 or max(shape) > MAX_SIDE or shape[0] * shape[1] > MAX_PIXELS:
        raise ValueError(f"{what}: a plane of shape {tuple(shape)}: sides in 1..{MAX_SIDE} and h * w <= {MAX_PIXELS}")


def patch_support_host(probs, cand, labels):
    """the numpy form of the support pass (``dt_patch_support``): fp32 ``[K, h, w]`` probabilities, the candidates' uint8 class
    map and its int32 label plane -> ``(roots, cls, qmax, qsum, area)``, one entry per patch in ascending root: ``roots``
    int64 (label - 1), ``cls`` uint8, and over the patch's pixels the maximum (int64), the sum (int64) and the count (int64)
    of ``q`` of the pixel's own class.  Integer arithmetic throughout"""
    probs = np.asarray(probs, dtype=np.float32)
    cand, labels = np.asarray(cand), np.asarray(labels)
    if probs.ndim != 3 or not 2 <= probs.shape[0] <= MAX_CLASSES:
        raise ValueError(f"patch_support_host: probs must be [K, h, w] with K in 2..{MAX_CLASSES}, got shape {probs.shape}")
    _check_plane_shape(probs.shape[1:], "patch_support_host")
    if cand.dtype != np.uint8 or labels.dtype != np.int32 or cand.shape != probs.shape[1:] or labels.shape != cand.shape:
        raise ValueError(f"patch_support_host: a uint8 class map and an int32 label plane of shape {probs.shape[1:]}, got "
                         f"{cand.dtype} {cand.shape} and {labels.dtype} {labels.shape}")
    if cand.size and int(cand.max()) >= probs.shape[0]:
        raise ValueError(f"patch_support_host: class value {int(cand.max())} out of range (K={probs.shape[0]})")
    own = np.take_along_axis(probs.reshape(probs.shape[0], -1), cand.reshape(1, -1).astype(np.int64), 0)[0]
    return patch_support_q_host(quantise(own), cand, labels)


def patch_support_q_host(q_own, cand, labels):
    """the integer core of ``patch_support_host``: ``q_own`` holds, per pixel, the ``q`` of the pixel's own class (any shape
    with ``labels.size`` elements; read on labelled pixels only) -> ``(roots, cls, qmax, qsum, area)``"""
    cand, labels = np.asarray(cand), np.asarray(labels)
    q_own = np.asarray(q_own).reshape(-1)
    flat = labels.ravel()
    at = np.flatnonzero(flat)
    if at.size == 0:
        empty = np.zeros(0, np.int64)
        return empty, np.zeros(0, np.uint8), empty.copy(), empty.copy(), empty.copy()
    q = q_own[at]
    order = np.argsort(flat[at], kind="stable")
    sorted_labels = flat[at][order]
    starts = np.flatnonzero(np.concatenate([[True], sorted_labels[1:] != sorted_labels[:-1]]))
    roots = sorted_labels[starts].astype(np.int64) - 1
    q = q[order].astype(np.int64)
    area = np.diff(np.concatenate([starts, [sorted_labels.size]])).astype(np.int64)
    return roots, cand.ravel()[roots], np.maximum.reduceat(q, starts), np.add.reduceat(q, starts), area


def decide_patchwise_host(probs, decision: Decision) -> np.ndarray:
    """the numpy form of ``ops.decide_patchwise``, the patch-wise rule of the contract: fp32 ``[K, h, w]`` probabilities ->
    uint8 ``[h, w]``.  Candidates at the low thresholds, their patches (``label_patches_host`` with the decision's
    connectivity), and a patch of class ``c`` is kept iff ``max q >= T_c`` and ``sum q >= M_c * area`` (64-bit integers);
    the pixels of every other patch become class 0"""
    from ..deployment.patches import label_patches_host
    probs = np.asarray(probs, dtype=np.float32)
    if probs.ndim != 3:
        raise ValueError(f"decide_patchwise_host: probs must be [K, h, w], got shape {probs.shape}")
    K = probs.shape[0]
    _check_plane_shape(probs.shape[1:], "decide_patchwise_host")
    T = decision.thresholds_u16(K).astype(np.int64)
    L, M = decision.low_u16(K), decision.min_confidence_u16(K).astype(np.int64)
    cand = decide_host(probs, Decision.from_q({c: int(L[c]) for c in range(1, K)}))
    labels = label_patches_host(cand, K, decision.connectivity)
    roots, cls, qmax, qsum, area = patch_support_host(probs, cand, labels)
    keep = (qmax >= T[cls]) & (qsum >= M[cls] * area)
    kept = np.zeros(labels.size + 1, bool)                      # by label; label 0 is background
    kept[roots[keep] + 1] = True
    return np.where(kept[labels], cand, 0).astype(np.uint8)
