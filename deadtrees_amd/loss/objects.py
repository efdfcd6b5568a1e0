"""Crown-level validation curves: what every hysteresis decision at one low threshold would find, counted in crowns.

``ProbabilityCurves.best_threshold`` optimises a pixel score; users of dead-tree maps count crowns.  For a fixed low
threshold ``L`` the extent of every hysteresis patch is fixed, and the high threshold ``T`` and the minimum mean confidence
``M`` of a ``Decision`` only decide whether a patch is kept: iff ``qmax >= T`` and ``qsum >= M * area``.  ONE labelling at
``L`` per validation batch therefore gives crown-level TP / FP / FN for all ``(T, M)`` at once, as a small integer histogram
that adds over images, batches, ranks and epochs.

The contract, in one place (the device path, ``csrc/objects.hip`` through ``ops.object_histogram``, computes
exactly this; ``object_histogram_host`` is the CPU path).  Everything is an integer: device and host compare with
``array_equal``.  Per image, for ``q`` uint16 ``[K, H, W]`` (the quantised probabilities of ``loss/curves.py``) and a target
``[H, W]``:

1. ``cand`` is the pixel rule at ``L``: the class ``c >= 1`` with the largest ``q_c`` among those with ``q_c >= L_c``, ties to
   the smallest ``c``, else 0 — ``decide_host`` at ``Decision.from_q(L)``; ``q_own`` is the winner's ``q``;
2. ``LP = label_patches_host(cand, K, connectivity)`` and ``LT = label_patches_host(target, K, connectivity)``; a target
   label outside ``[0, K)`` raises the error flag and counts as background, as in ``dt_prob_histogram``;
3. per predicted patch ``qmax``, ``S = sum q_own`` (int64) and the area ``A`` (``patch_support_host``'s integer core); a patch
   with ``A < min_pixels`` does not exist;
4. a target patch ``a`` and a predicted patch ``b`` of the SAME class match iff ``n * q > p * (A_a + A_b - n)`` in int64,
   ``n`` their shared pixel count and ``p / q = min_iou >= 1/2``.  The rule is STRICTLY above ``min_iou``, on purpose: above
   1/2 a patch has at most one partner, so the matching is unique and needs no greedy order; at exactly 1/2 it is not
   (``PatchOverlaps.match`` documents the same boundary).  ``PatchOverlaps.match`` itself accepts ``IoU >= min_iou``: a
   pair at exactly ``min_iou`` matches there and not here;
5. ``hist`` int64 ``[K, 2, 256, 256]``, indexed ``[c, m, jT, jM]``, gets one entry per predicted patch: ``m = 1`` iff the
   patch is matched, ``jT = qmax >> 8``, ``jM = (S // A) >> 8``; ``targets`` int64 ``[K]`` counts the target patches per
   class.  Row and entry 0 stay zero.

Reading the histogram (``ObjectCurves``): threshold index ``j`` means ``T = 256 j``, index ``i`` means ``M = 256 i`` and
``i = 0`` no filter; a patch is kept at ``(j, i)`` iff ``jT >= j`` and ``jM >= i`` — exact, because ``S >= M * A`` iff
``S // A >= M`` for an integer ``M``.  Closure, bit for bit and for every K: for ``256 j >= L_c`` the counts at ``(j, i)`` are
those of ``decide_patchwise_host`` with ``Decision.from_q({c: 256 j}, low=L, min_confidence={c: 256 i})``, then
``sieve_host(min_pixels)``, ``overlap_pairs_host`` against the target's label plane and the strict IoU filter with equal
classes, summed over the images.

Out of scope: a plane masked by ``lu``, sweeps over ``L`` inside one pass (one ``ObjectSweep`` per ``L``),
``same_class=False``, decisions stored in checkpoints, a raster-level ``infer_tile`` option (``ops.object_histogram`` takes
``B = 1`` planes).

numpy and the standard library only (``label_patches_host`` imports scipy lazily).
"""
from __future__ import annotations

from fractions import Fraction
from typing import Mapping, Optional, Sequence, Tuple

import numpy as np

from .curves import BINS, Decision, _class_thresholds, patch_support_q_host
from ..deployment.attributes import Q_SCALE

MAX_DENOMINATOR = 10 ** 6
FALLBACK_T = 32768                       # the threshold of a class whose curves say nothing: the arg-max of K = 2


class ObjectSweep:
    """what one crown-level sweep fixes: the low thresholds ``L_c`` of exactly the classes ``1..K-1`` (parsed like a
    ``Decision`` threshold: a float in ``(0, 1]`` is ``floor(t * 65535 + 0.5)``, an int is a ``q`` in ``1..65535``;
    ``ObjectSweep.from_q`` takes integers only), the ``connectivity`` (4 or 8) of predicted and target patches, ``min_pixels
    >= 0`` (predicted patches with fewer pixels are dropped before matching) and ``min_iou`` in ``[0.5, 1)``, taken as
    ``p / q = Fraction(min_iou).limit_denominator(10**6)``; a pair matches STRICTLY above it."""

    def __init__(self, low: Mapping[int, float], connectivity: int = 8, min_pixels: int = 0, min_iou=0.5):
        if not isinstance(low, Mapping) or not low:
            raise ValueError(f"ObjectSweep: low must be a non-empty mapping class -> threshold, got {low!r}")
        try:
            self.low = _class_thresholds(low, "low")
        except ValueError as e:
            raise ValueError("ObjectSweep: " + str(e).split(": ", 1)[-1]) from None
        missing = sorted(set(range(1, max(self.low) + 1)) - set(self.low))
        if missing:
            raise ValueError(f"ObjectSweep: no low threshold for class(es) {missing}: every class 1..K-1 must be named")
        if isinstance(connectivity, (bool, np.bool_)) or connectivity not in (4, 8):
            raise ValueError(f"ObjectSweep: connectivity must be 4 or 8, got {connectivity!r}")
        self.connectivity = int(connectivity)
        if isinstance(min_pixels, (bool, np.bool_)) or not isinstance(min_pixels, (int, np.integer)) or min_pixels < 0:
            raise ValueError(f"ObjectSweep: min_pixels must be an integer >= 0, got {min_pixels!r}")
        self.min_pixels = int(min_pixels)
        if isinstance(min_iou, (bool, np.bool_)) or not isinstance(min_iou, (int, float, np.integer, np.floating, Fraction)) \
                or not 0.5 <= min_iou < 1:                           # (nan fails too)
            raise ValueError(f"ObjectSweep: min_iou must lie in [0.5, 1), got {min_iou!r}")
        iou = Fraction(float(min_iou) if isinstance(min_iou, (np.floating, np.integer)) else min_iou)
        iou = iou.limit_denominator(MAX_DENOMINATOR)
        if not Fraction(1, 2) <= iou < 1:
            raise ValueError(f"ObjectSweep: min_iou {min_iou!r} is {iou} with a denominator of at most {MAX_DENOMINATOR}: "
                             "it must lie in [0.5, 1)")
        self.iou_p, self.iou_q = int(iou.numerator), int(iou.denominator)

    @classmethod
    def from_q(cls, low: Mapping[int, int], connectivity: int = 8, min_pixels: int = 0, min_iou=0.5) -> "ObjectSweep":
        """low thresholds given as integers ``L`` on the ``q`` axis, taken as they are"""
        if isinstance(low, Mapping):
            for c, t in low.items():
                if isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, np.integer)):
                    raise ValueError(f"ObjectSweep.from_q: threshold {t!r} of class {c!r} is not an integer")
        return cls(low, connectivity=connectivity, min_pixels=min_pixels, min_iou=min_iou)

    @property
    def K(self) -> int:
        return len(self.low) + 1

    @property
    def min_iou(self) -> Fraction:
        return Fraction(self.iou_p, self.iou_q)

    def low_u16(self, K: Optional[int] = None) -> np.ndarray:
        """uint16 [K]: ``L_c`` at index ``c``, 0 (not read) at index 0; a ``K`` other than this sweep's is a ``ValueError``"""
        if K is not None and int(K) != self.K:
            raise ValueError(f"ObjectSweep: low thresholds for the classes 1..{self.K - 1}, but K={K}: every class 1..K-1 must "
                             "be named, and no other")
        return np.array([0] + [self.low[c] for c in range(1, self.K)], dtype=np.uint16)

    def _key(self):
        return tuple(sorted(self.low.items())), self.connectivity, self.min_pixels, self.iou_p, self.iou_q

    def __eq__(self, other) -> bool:
        if not isinstance(other, ObjectSweep):
            return NotImplemented
        return self._key() == other._key()

    __hash__ = None

    def __repr__(self) -> str:
        return (f"ObjectSweep.from_q({self.low!r}, connectivity={self.connectivity}, min_pixels={self.min_pixels}, "
                f"min_iou=Fraction({self.iou_p}, {self.iou_q}))")


def check_sweep(option, K: Optional[int], caller: str) -> Optional[ObjectSweep]:
    """the ``objects`` argument of ``validate`` / ``fit`` -> ``ObjectSweep`` or None; a wrong type or a class set other
    than ``1..K-1`` is a ``ValueError`` naming the caller"""
    if option is None:
        return None
    if not isinstance(option, ObjectSweep):
        raise ValueError(f"{caller}: objects must be an ObjectSweep or None, got {option!r}")
    if K is not None and option.K != int(K):
        raise ValueError(f"{caller}: objects names the classes 1..{option.K - 1}, the model has the classes 1..{int(K) - 1}")
    return option


def candidates_host(q, low_u16) -> Tuple[np.ndarray, np.ndarray]:
    """step 1 of the contract on integers: ``q`` ``[K, ...]`` -> ``(cand uint8 [...], q_own int64 [...])``"""
    q = np.asarray(q).astype(np.int64)
    L = np.asarray(low_u16).astype(np.int64)
    above = np.where(q[1:] >= L[1:].reshape((-1,) + (1,) * (q.ndim - 1)), q[1:], -1)
    best = np.argmax(above, axis=0)                               # the first of equal maxima: the smallest class
    top = np.take_along_axis(above, best[None], 0)[0]
    return np.where(top >= 0, best + 1, 0).astype(np.uint8), np.where(top >= 0, top, 0)


def object_histogram_host(q, target, sweep: ObjectSweep):
    """the numpy oracle of ``ops.object_histogram``: ``q`` integers ``[B, K, H, W]`` in ``0..65535``, ``target`` integers
    ``[B, H, W]`` -> ``(hist int64 [K, 2, 256, 256], targets int64 [K], err)``; ``err`` is 1 when a target label lies outside
    ``[0, K)``.  A loop over the images"""
    from ..deployment.overlaps import overlap_pairs_host
    from ..deployment.patches import label_patches_host
    if not isinstance(sweep, ObjectSweep):
        raise ValueError(f"object_histogram_host: sweep must be an ObjectSweep, got {sweep!r}")
    q, target = np.asarray(q), np.asarray(target)
    if q.ndim != 4 or not np.issubdtype(q.dtype, np.integer) or q.size == 0:
        raise ValueError(f"object_histogram_host: q must be non-empty integers [B, K, H, W], got {q.dtype} {q.shape}")
    B, K, H, W = q.shape
    if target.shape != (B, H, W) or not np.issubdtype(target.dtype, np.integer):
        raise ValueError(f"object_histogram_host: target must be integers {(B, H, W)}, got {target.dtype} {target.shape}")
    if q.min() < 0 or q.max() > Q_SCALE:
        raise ValueError(f"object_histogram_host: q outside 0..{Q_SCALE}")
    L = sweep.low_u16(K)
    p, r = sweep.iou_p, sweep.iou_q
    hist = np.zeros((K, 2, BINS, BINS), dtype=np.int64)
    targets = np.zeros(K, dtype=np.int64)
    valid = (target >= 0) & (target < K)
    for b in range(B):
        cand, q_own = candidates_host(q[b], L)
        tcls = np.where(valid[b], target[b], 0).astype(np.uint8)
        LP = label_patches_host(cand, K, sweep.connectivity)
        LT = label_patches_host(tcls, K, sweep.connectivity)
        roots, cls, qmax, qsum, area = patch_support_q_host(q_own, cand, LP)
        exists = area >= sweep.min_pixels
        t_labels, t_area = np.unique(LT[LT > 0], return_counts=True)
        t_roots = t_labels.astype(np.int64) - 1
        t_cls = tcls.ravel()[t_roots]
        targets += np.bincount(t_cls, minlength=K).astype(np.int64)
        matched = np.zeros(len(roots), dtype=np.int64)
        pa, pb, n = overlap_pairs_host(LT, LP)
        if len(pa):
            ia, ib = np.searchsorted(t_roots, pa), np.searchsorted(roots, pb)
            union = t_area[ia].astype(np.int64) + area[ib] - n
            hit = (t_cls[ia] == cls[ib]) & exists[ib] & (n * r > p * union)
            matched[ib[hit]] = 1
        np.add.at(hist, (cls[exists].astype(np.int64), matched[exists], qmax[exists] >> 8, (qsum[exists] // area[exists]) >> 8), 1)
    return hist, targets, int(not valid.all())


class ObjectCurves:
    """the crown-level curves of one histogram ``[K, 2, 256, 256]`` and its target counts ``[K]``, for the ``ObjectSweep`` that
    collected them.  Arrays are read-only; ``+`` adds two epochs, ranks or batches of EQUAL sweeps.  Threshold index ``j``
    means ``T = 256 j``, ``i`` means ``M = 256 i`` (``i = 0``: no filter); a class without targets gives ``nan``, never an
    exception."""

    def __init__(self, hist, targets, sweep: ObjectSweep, class_names: Optional[Sequence[str]] = None):
        if not isinstance(sweep, ObjectSweep):
            raise ValueError(f"ObjectCurves: sweep must be an ObjectSweep, got {sweep!r}")
        hist, targets = np.asarray(hist), np.asarray(targets)
        if hist.ndim != 4 or hist.shape[1:] != (2, BINS, BINS) or hist.shape[0] != sweep.K:
            raise ValueError(f"ObjectCurves: hist must be [{sweep.K}, 2, {BINS}, {BINS}] for this sweep, got {hist.shape}")
        if targets.shape != (sweep.K,):
            raise ValueError(f"ObjectCurves: targets must be [{sweep.K}], got {targets.shape}")
        for name, a in (("hist", hist), ("targets", targets)):
            if not np.issubdtype(a.dtype, np.integer) and not np.array_equal(a, np.floor(a)):
                raise ValueError(f"ObjectCurves: {name} holds counts: integers")
            if (a < 0).any():
                raise ValueError(f"ObjectCurves: {name} must not be negative")
        self.hist, self.targets = hist.astype(np.int64), targets.astype(np.int64)
        if self.hist[0].any() or self.targets[0]:
            raise ValueError("ObjectCurves: class 0 has no patches: row 0 of hist and entry 0 of targets are zero")
        self.hist.setflags(write=False)
        self.targets.setflags(write=False)
        self.sweep, self.K = sweep, sweep.K
        if class_names is not None:
            class_names = tuple(str(n) for n in class_names)
            if len(class_names) != self.K:
                raise ValueError(f"ObjectCurves: {len(class_names)} class names for K={self.K}")
        self.class_names = class_names

    def __add__(self, other):
        if not isinstance(other, ObjectCurves):
            return NotImplemented
        if other.sweep != self.sweep:
            raise ValueError(f"ObjectCurves: {self.sweep!r} + {other.sweep!r}: the sweeps must be equal")
        return ObjectCurves(self.hist + other.hist, self.targets + other.targets, self.sweep,
                            self.class_names if self.class_names is not None else other.class_names)

    def __eq__(self, other) -> bool:
        if not isinstance(other, ObjectCurves):
            return NotImplemented
        return self.sweep == other.sweep and np.array_equal(self.hist, other.hist) and np.array_equal(self.targets, other.targets)

    __hash__ = None

    def __repr__(self) -> str:
        names = "" if self.class_names is None else f", classes={list(self.class_names)}"
        return (f"ObjectCurves(K={self.K}, patches={int(self.hist.sum())}, targets={int(self.targets.sum())}, "
                f"sweep={self.sweep!r}{names})")

    def _class(self, c) -> int:
        if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 1 <= c < self.K:
            raise ValueError(f"ObjectCurves: class {c!r} is not in 1..{self.K - 1}")
        return int(c)

    @staticmethod
    def _index(i) -> int:
        if isinstance(i, bool) or not isinstance(i, (int, np.integer)) or not 0 <= i < BINS:
            raise ValueError(f"ObjectCurves: confidence index {i!r} is not in 0..{BINS - 1}")
        return int(i)

    # ------------------------------------------------------------------ counts per (j, i)
    def counts2d(self, c: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """``(tp, fp, fn)`` int64 [256, 256] over ``(j, i)``: the patches with ``jT >= j`` and ``jM >= i``, matched / not, and
        ``fn = targets[c] - tp`` (above an IoU of 1/2 a matched patch is exactly one found crown)"""
        c = self._class(c)
        tail = lambda h: np.cumsum(np.cumsum(h[::-1, ::-1], axis=0), axis=1)[::-1, ::-1].astype(np.int64)   # noqa: E731
        tp, fp = tail(self.hist[c, 1]), tail(self.hist[c, 0])
        return tp, fp, self.targets[c] - tp

    def counts(self, c: int, i: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """``(tp, fp, fn)`` int64 [256] over ``j`` at the confidence index ``i``"""
        i = self._index(i)
        return tuple(a[:, i].copy() for a in self.counts2d(c))

    def precision_recall(self, c: int, i: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """``(precision, recall)`` fp64 [256]; precision is 1.0 where no patch is kept, recall ``nan`` without targets"""
        tp, fp, _ = self.counts(c, i)
        kept, pos = tp + fp, int(self.targets[self._class(c)])
        precision = np.where(kept > 0, tp / np.maximum(kept, 1), 1.0)
        recall = tp / pos if pos > 0 else np.full(tp.shape, np.nan)
        return precision, recall

    def average_precision(self, c: int, i: int = 0) -> float:
        """the step sum ``sum_j (R_j - R_{j+1}) * P_j`` over ``j = 0..255`` with ``R_256 = 0`` (nothing is kept), as
        ``ProbabilityCurves.average_precision``; ``nan`` without targets"""
        precision, recall = self.precision_recall(c, i)
        recall = np.concatenate([recall, [0.0]])
        return float(np.sum((recall[:-1] - recall[1:]) * precision))

    def f1(self, c: int) -> np.ndarray:
        """fp64 [256, 256]: ``2 tp / (2 tp + fp + fn)``; ``nan`` without targets"""
        tp, fp, fn = self.counts2d(c)
        if int(self.targets[self._class(c)]) == 0:
            return np.full(tp.shape, np.nan)
        return 2.0 * tp / (2 * tp + fp + fn)

    def _best(self, c: int):
        """``(j, i, f1)`` of the largest F1 among the ``j`` with ``256 j >= L_c``, ties to the smallest ``j``, then the
        smallest ``i``; ``(None, None, nan)`` without targets or without such a ``j``"""
        c = self._class(c)
        first = -(-self.sweep.low[c] // BINS)                       # ceil(L_c / 256) >= 1
        if int(self.targets[c]) == 0 or first >= BINS:
            return None, None, float("nan")
        score = self.f1(c)[first:]
        at = int(np.argmax(score))                                  # row-major: the first of equal maxima
        return first + at // BINS, at % BINS, float(score.reshape(-1)[at])

    def best_decision(self) -> Decision:
        """the ``Decision`` of largest crown-level F1 per class: ``T = 256 j``, ``low = L``, ``min_confidence = 256 i`` only
        where ``i > 0``, the sweep's connectivity.  A class without targets (or with ``L_c > 65280``: no ``j`` above it)
        keeps ``T = max(L_c, 32768)``"""
        T, M = {}, {}
        for c in range(1, self.K):
            j, i, _ = self._best(c)
            T[c] = max(self.sweep.low[c], FALLBACK_T) if j is None else BINS * j
            if i:
                M[c] = BINS * i
        return Decision.from_q(T, low=dict(self.sweep.low), min_confidence=M or None, connectivity=self.sweep.connectivity)

    def summary(self, prefix: str = "val") -> dict:
        """the scalars ``fit`` logs, for every class ``c >= 1``: ``{prefix}/crown_ap_<c>`` (at ``i = 0``), ``/crown_best_f1_<c>``
        (``nan`` without targets), ``/crown_best_threshold_<c>`` and ``/crown_best_min_confidence_<c>`` (the floats
        ``T / 65535`` and ``M / 65535`` of ``best_decision``; 0.0: no filter) and ``/crown_targets_<c>``"""
        out, best = {}, self.best_decision()
        for c in range(1, self.K):
            out[f"{prefix}/crown_ap_{c}"] = self.average_precision(c)
            out[f"{prefix}/crown_best_f1_{c}"] = self._best(c)[2]
            out[f"{prefix}/crown_best_threshold_{c}"] = best.q[c] / Q_SCALE
            out[f"{prefix}/crown_best_min_confidence_{c}"] = best.min_confidence.get(c, 0) / Q_SCALE
            out[f"{prefix}/crown_targets_{c}"] = float(self.targets[c])
        return out


def crown_monitors(K: int, stage: str = "val") -> tuple:
    """the crown-level scalars a checkpoint or early-stopping monitor may name when ``fit`` runs with ``objects``"""
    return tuple(f"{stage}/crown_{name}_{c}" for c in range(1, int(K)) for name in ("best_f1", "ap"))
