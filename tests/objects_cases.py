"""Inputs and the yardstick chain shared by tests/test_objects_host.py and tests/test_objects_gpu.py (no tests here).

``blobs`` draws smooth random quantised probabilities and a target that resembles them without being them; ``chain_counts``
is the closure of ``loss/objects.py`` spelled with the functions that existed before it: ``decide_patchwise_host``, then
``sieve_host``, then ``overlap_pairs_host`` against the target's label plane, then the strict IoU filter with equal classes."""
import numpy as np

from deadtrees_amd.deployment.overlaps import overlap_pairs_host
from deadtrees_amd.deployment.patches import label_patches_host, sieve_host
from deadtrees_amd.loss.curves import Decision, decide_patchwise_host, quantise

# seeds at which B = 3, 19 x 33 holds at least one TP, one FP and one FN per class (the tests assert it)
CLOSURE_SEEDS = {2: 3, 3: 5}
LOW = {1: 20000, 2: 17000, 3: 21000, 4: 19000, 5: 18000, 6: 22000, 7: 16000}


def low_for(K):
    return {c: LOW[c] for c in range(1, K)}


def blobs(seed, B, K, H, W, sigma=2.0):
    """``(q uint16 [B, K, H, W], target int64 [B, H, W])``: per class a smooth field; the target thresholds the field plus a
    smooth disturbance, so crowns are found, missed, split and invented"""
    from scipy import ndimage
    rng = np.random.default_rng(seed)

    def smooth(shape):
        f = ndimage.gaussian_filter(rng.standard_normal(shape), sigma=(0, 0, sigma, sigma), mode="constant")
        return f / max(float(np.abs(f).max()), 1e-9)

    f = smooth((B, K, H, W))
    g = f + 0.3 * smooth((B, K, H, W))
    q = np.clip(np.floor((0.25 + 0.9 * f) * 65535 + 0.5), 0, 65535).astype(np.uint16)
    q[:, 0] = 65535 - q[:, 1:].max(1)
    top = g[:, 1:].argmax(1) + 1
    target = np.where(g[:, 1:].max(1) > 0.12, top, 0).astype(np.int64)
    return q, target


def probs_of(q):
    """fp32 probabilities whose quantisation IS ``q`` (checked): what the host functions that take probabilities are given"""
    p = (np.asarray(q).astype(np.float64) / 65535.0).astype(np.float32)
    assert np.array_equal(quantise(p), np.asarray(q).astype(np.int64))
    return p


def chain_counts(q, target, sweep, c, j, i):
    """``(tp, fp, fn)`` of class ``c`` at ``T = 256 j``, ``M = 256 i`` through the existing chain, summed over the images"""
    B, K = q.shape[:2]
    T = dict(sweep.low)
    T[c] = 256 * j
    d = Decision.from_q(T, low=dict(sweep.low), min_confidence={c: 256 * i} if i else None, connectivity=sweep.connectivity)
    p, r = sweep.iou_p, sweep.iou_q
    tp = kept = crowns = 0
    for b in range(B):
        decided = decide_patchwise_host(probs_of(q[b]), d)
        decided, labels = sieve_host(decided, label_patches_host(decided, K, sweep.connectivity), sweep.min_pixels)
        tcls = np.where((target[b] >= 0) & (target[b] < K), target[b], 0).astype(np.uint8)
        LT = label_patches_host(tcls, K, sweep.connectivity)
        area_t, area_p = np.bincount(LT.ravel()), np.bincount(labels.ravel())
        roots_t, roots_p = np.unique(LT[LT > 0]) - 1, np.unique(labels[labels > 0]) - 1
        crowns += int((tcls.ravel()[roots_t] == c).sum())
        kept += int((decided.ravel()[roots_p] == c).sum())
        pa, pb, n = overlap_pairs_host(LT, labels)
        union = area_t[pa + 1] + area_p[pb + 1] - n
        same = (tcls.ravel()[pa] == c) & (decided.ravel()[pb] == c)
        tp += int((same & (n * r > p * union)).sum())
    return tp, kept - tp, crowns - tp


def sampled_points(rng, L_c, n=12):
    """at least ``n`` pairs ``(j, i)`` with ``256 j >= L_c``, ``j = ceil(L_c / 256)`` and ``i = 0`` among them"""
    first = -(-L_c // 256)
    pts = {(first, 0), (first, int(rng.integers(1, 256))), (int(rng.integers(first, 256)), 0), (255, 0), (255, 255)}
    while len(pts) < n:
        pts.add((int(rng.integers(first, 256)), int(rng.integers(0, 256))))
    return sorted(pts)
