"""Inputs shared by tests/test_hysteresis_host.py and tests/test_hysteresis_gpu.py: the random probability fields of the
patch-wise decision, the conditions a field case must meet on the host rule before anything is compared with it, and the
hand-computed 6 x 8 example.  numpy and scipy only; no test lives here."""
import functools

import numpy as np

Q = 65535
LOW, HIGH, MEAN = 20000, 36000, 27000            # L, T and M of every field case, on the q axis
FIELD_SHAPES = ((64, 200), (131, 257))


@functools.lru_cache(maxsize=None)
def field(K, h, w):
    """fp32 [K, h, w] (read-only): K independent standard-normal planes from ``default_rng(7 + K)``, each smoothed with a
    Gaussian of sigma 3 and multiplied by 12, plane 0 raised by 1.0, cast to float32, then a float32 softmax over K"""
    from scipy import ndimage
    z = np.random.default_rng(7 + K).standard_normal((K, h, w))
    z = np.stack([ndimage.gaussian_filter(z[k], sigma=3) for k in range(K)]) * 12
    z[0] += 1.0
    z = z.astype(np.float32)
    e = np.exp(z - z.max(axis=0, keepdims=True))
    p = (e / e.sum(axis=0, keepdims=True, dtype=np.float32)).astype(np.float32)
    p.setflags(write=False)
    return p


def decision(K, connectivity, with_mean):
    from deadtrees_amd.loss.curves import Decision
    classes = range(1, K)
    return Decision.from_q({c: HIGH for c in classes}, low={c: LOW for c in classes},
                           min_confidence={c: MEAN for c in classes} if with_mean else None, connectivity=connectivity)


def patch_fates(p, dec):
    """(cls, core, mean) per candidate patch of the host rule: its class, whether ``qmax >= T`` and whether ``S >= M * A``"""
    from deadtrees_amd.deployment.patches import label_patches_host
    from deadtrees_amd.loss.curves import Decision, decide_host, patch_support_host
    K = p.shape[0]
    cand = decide_host(p, Decision.from_q({c: int(dec.low_u16(K)[c]) for c in range(1, K)}))
    _, cls, qmax, qsum, area = patch_support_host(p, cand, label_patches_host(cand, K, dec.connectivity))
    T, M = dec.thresholds_u16(K).astype(np.int64), dec.min_confidence_u16(K).astype(np.int64)
    return cls, qmax >= T[cls], qsum >= M[cls] * area


def assert_not_degenerate(p, dec):
    """every class has at least one kept and one rejected patch; at 131 x 257 the M filter rejects a patch that T keeps.
    The one field that cannot meet the second condition is K = 3 under connectivity 8: there every patch with a core has
    the mean as well (under connectivity 4 one does not), so that case checks the M arithmetic on kept patches only"""
    cls, core, mean = patch_fates(p, dec)
    kept = core & mean
    for c in range(1, p.shape[0]):
        assert (kept & (cls == c)).any() and (~kept & (cls == c)).any(), (c, p.shape, dec)
    if dec.min_confidence and p.shape[1:] == (131, 257) and (p.shape[0], dec.connectivity) != (3, 8):
        assert (core & ~mean).any(), (p.shape, dec)


# ---------------------------------------------------------------------- the hand-computed example (K = 2)
# l: a candidate below T; H: a pixel at T; .: background.  A (rows 0-1) holds an H.  B is the diagonal chain (1,5) - (2,4) -
# (3,3) with its H at the far end: one patch under connectivity 8, three single pixels under 4.  C and D hold no H.
HAND_L, HAND_T = 20000, 40000
_l, _H, _o = HAND_L, HAND_T, 1000
HAND_Q1 = np.array([[_o, _l, _l, _o, _o, _o, _o, _o],
                    [_o, _l, _H, _o, _o, _l, _o, _o],
                    [_o, _o, _o, _o, _l, _o, _o, _o],
                    [_o, _o, _o, _H, _o, _o, _o, _o],
                    [_l, _o, _o, _o, _o, _o, _l, _l],
                    [_l, _l, _o, _o, _o, _o, _o, _l]], dtype=np.int64)
HAND_WANT = {8: np.array([[0, 1, 1, 0, 0, 0, 0, 0],
                          [0, 1, 1, 0, 0, 1, 0, 0],
                          [0, 0, 0, 0, 1, 0, 0, 0],
                          [0, 0, 0, 1, 0, 0, 0, 0],
                          [0, 0, 0, 0, 0, 0, 0, 0],
                          [0, 0, 0, 0, 0, 0, 0, 0]], dtype=np.uint8),
             4: np.array([[0, 1, 1, 0, 0, 0, 0, 0],
                          [0, 1, 1, 0, 0, 0, 0, 0],
                          [0, 0, 0, 0, 0, 0, 0, 0],
                          [0, 0, 0, 1, 0, 0, 0, 0],
                          [0, 0, 0, 0, 0, 0, 0, 0],
                          [0, 0, 0, 0, 0, 0, 0, 0]], dtype=np.uint8)}


def probs_of_q(q1):
    """fp32 [2, ...]: class 1 has probability ``float32(q / 65535)``, class 0 the rest"""
    p1 = (np.asarray(q1, dtype=np.float64) / Q).astype(np.float32)
    return np.stack([(1 - p1).astype(np.float32), p1])
