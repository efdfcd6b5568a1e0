"""The patch-wise decision on the host (``deadtrees_amd/loss/curves.py``): the arguments of ``Decision``, the rule on a
hand-computed example and on both sides of its integer boundaries, out-of-range probabilities, and the properties of the
contract on random fields, checked against a flood fill written here.  Every comparison is ``array_equal``."""
import numpy as np
import pytest

import hysteresis_cases as hc
from deadtrees_amd.deployment.patches import label_patches_host
from deadtrees_amd.loss.curves import Decision, decide_host, decide_patchwise_host, patch_support_host, quantise


# ---------------------------------------------------------------------- Decision
def test_decision_arguments():
    d = Decision({1: 0.5, 2: 40000}, low={1: 0.25, 2: 40000}, min_confidence={2: 0.5}, connectivity=4)
    assert d.K == 3 and d.patchwise and d.connectivity == 4
    assert d.thresholds_u16(3).tolist() == [0, 32768, 40000] and d.thresholds_u16().dtype == np.uint16
    assert d.low_u16(3).tolist() == [0, 16384, 40000] and d.low_u16().dtype == np.uint16
    assert d.min_confidence_u16(3).tolist() == [0, 0, 32768] and d.min_confidence_u16().dtype == np.uint16
    for accessor in (d.thresholds_u16, d.low_u16, d.min_confidence_u16):
        with pytest.raises(ValueError, match="K=2"):
            accessor(2)
    same = Decision.from_q({1: 32768, 2: 40000}, low={1: 16384, 2: 40000}, min_confidence={2: 32768}, connectivity=4)
    assert d == same and eval(repr(d)) == d
    assert repr(d) == "Decision.from_q({1: 32768, 2: 40000}, low={1: 16384, 2: 40000}, min_confidence={2: 32768}, connectivity=4)"
    for other in (Decision({1: 0.5, 2: 40000}),
                  Decision.from_q({1: 32768, 2: 40000}, low={1: 16384, 2: 40000}, min_confidence={2: 32768}),
                  Decision.from_q({1: 32768, 2: 40000}, low={1: 16385, 2: 40000}, min_confidence={2: 32768}, connectivity=4),
                  Decision.from_q({1: 32768, 2: 40000}, low={1: 16384, 2: 40000}, min_confidence={1: 32768}, connectivity=4),
                  Decision.from_q({1: 32768, 2: 40000}, low={1: 16384, 2: 40000}, connectivity=4)):
        assert d != other
    only_mean = Decision({1: 0.5}, min_confidence={1: 0.75})
    assert only_mean.patchwise and only_mean.low_u16().tolist() == [0, 32768]
    assert repr(only_mean) == "Decision.from_q({1: 32768}, min_confidence={1: 49151}, connectivity=8)"
    assert eval(repr(only_mean)) == only_mean
    assert Decision({1: 0.5}, low={1: 1}).low_u16().tolist() == [0, 1]          # an int is a q


def test_a_decision_that_is_not_patchwise_is_the_plain_one():
    plain = Decision({1: .5})
    for d in (Decision({1: .5}, low={1: .5}), Decision({1: .5}, low=None, min_confidence={}, connectivity=4),
              Decision.from_q({1: 32768}, low={1: 32768})):
        assert not d.patchwise and d == plain and plain == d and repr(d) == repr(plain) == "Decision.from_q({1: 32768})"
        assert d.low_u16(2).tolist() == d.thresholds_u16(2).tolist() and d.min_confidence_u16(2).tolist() == [0, 0]
    assert not plain.patchwise and plain.connectivity == 8


def test_decision_errors():
    with pytest.raises(ValueError, match="low threshold above"):
        Decision({1: 0.3}, low={1: 0.31})
    with pytest.raises(ValueError, match="low threshold above"):
        Decision.from_q({1: 100, 2: 100}, low={1: 100, 2: 101})
    for low in ({2: 0.1}, {1: 0.1, 2: 0.1}, {}):                  # another class set
        with pytest.raises(ValueError, match="must be the same"):
            Decision({1: 0.3}, low=low)
    with pytest.raises(ValueError, match="min_confidence names"):
        Decision({1: 0.3}, min_confidence={2: 0.3})
    for conn in (3, 6, True, "8", None, 8.5):
        with pytest.raises(ValueError, match="connectivity"):
            Decision({1: 0.3}, connectivity=conn)
    for bad in (True, np.bool_(True), 0, 65536, 0.0, 1.5, float("nan"), "0.5", None):
        with pytest.raises(ValueError, match="threshold"):
            Decision({1: 0.9}, low={1: bad})
        with pytest.raises(ValueError, match="threshold"):
            Decision({1: 0.9}, min_confidence={1: bad})
    for key in ("low", "min_confidence"):
        with pytest.raises(ValueError, match="not an integer"):
            Decision.from_q({1: 100}, **{key: {1: 0.001}})
        with pytest.raises(ValueError, match="not an integer"):
            Decision.from_q({1: 100}, **{key: {1: True}})
        with pytest.raises(ValueError, match="mapping"):
            Decision({1: 0.5}, **{key: [0.1]})


# ---------------------------------------------------------------------- the rule, written out
def _flood_rule(p, dec):
    """the rule of the contract with a flood fill and Python integers: nothing of the module but ``quantise``"""
    K, h, w = p.shape
    q = quantise(p)
    T, L, M = ([int(v) for v in a(K)] for a in (dec.thresholds_u16, dec.low_u16, dec.min_confidence_u16))
    cand = np.zeros((h, w), np.uint8)
    for y in range(h):
        for x in range(w):
            best = -1
            for c in range(1, K):
                if q[c, y, x] >= L[c] and q[c, y, x] > best:
                    cand[y, x], best = c, int(q[c, y, x])
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if dec.connectivity == 8 else [])
    out, seen = np.zeros((h, w), np.uint8), np.zeros((h, w), bool)
    for y in range(h):
        for x in range(w):
            if cand[y, x] == 0 or seen[y, x]:
                continue
            c, stack, patch = int(cand[y, x]), [(y, x)], []
            seen[y, x] = True
            while stack:
                a, b = stack.pop()
                patch.append((a, b))
                for dy, dx in steps:
                    u, v = a + dy, b + dx
                    if 0 <= u < h and 0 <= v < w and not seen[u, v] and cand[u, v] == c:
                        seen[u, v] = True
                        stack.append((u, v))
            own = [int(q[c, a, b]) for a, b in patch]
            if max(own) >= T[c] and sum(own) >= M[c] * len(own):
                for a, b in patch:
                    out[a, b] = c
    return out


def test_the_hand_computed_example():
    p = hc.probs_of_q(hc.HAND_Q1)
    assert np.array_equal(quantise(p[1]), hc.HAND_Q1)
    for conn in (8, 4):
        dec = Decision.from_q({1: hc.HAND_T}, low={1: hc.HAND_L}, connectivity=conn)
        got = decide_patchwise_host(p, dec)
        assert got.dtype == np.uint8 and np.array_equal(got, hc.HAND_WANT[conn])
        assert np.array_equal(_flood_rule(p, dec), hc.HAND_WANT[conn])
    # the support of the candidates' patches under connectivity 8: A (4 pixels, one at T), the chain B, then C and D
    cand = decide_host(p, Decision.from_q({1: hc.HAND_L}))
    roots, cls, qmax, qsum, area = patch_support_host(p, cand, label_patches_host(cand, 2, 8))
    assert roots.tolist() == [1, 13, 32, 38] and cls.tolist() == [1, 1, 1, 1] and qsum.dtype == np.int64
    assert qmax.tolist() == [40000, 40000, 20000, 20000] and qsum.tolist() == [100000, 80000, 60000, 60000]
    assert area.tolist() == [4, 3, 3, 3]
    # the mean of A is 25000, that of B 26666.67: M = 25001 rejects A alone, M = 26667 both
    a = hc.HAND_WANT[8].copy()
    a[:, 4:] = 0
    a[2:] = 0
    b = hc.HAND_WANT[8] - a
    for M, want in ((25000, a + b), (25001, b), (26666, b), (26667, 0 * b)):
        dec = Decision.from_q({1: hc.HAND_T}, low={1: hc.HAND_L}, min_confidence={1: M})
        assert np.array_equal(decide_patchwise_host(p, dec), want), M


def test_both_sides_of_the_integer_boundaries():
    T, L = 30000, 10000
    for strong, kept in ((T, True), (T - 1, False), (T + 1, True)):
        p = hc.probs_of_q([[L, strong, L, 0, L]])
        assert np.array_equal(quantise(p[1]), [[L, strong, L, 0, L]])
        got = decide_patchwise_host(p, Decision.from_q({1: T}, low={1: L}))
        assert got.tolist() == [[1, 1, 1, 0, 0]] if kept else not got.any(), strong
    # S == M * A is kept, S == M * A - 1 rejected: three pixels, M = 20000, S = 60000 or 59999
    for q3, kept in (((T, 15000, 15000), True), ((T, 15000, 14999), False), ((T, 15001, 14999), True)):
        p = hc.probs_of_q([list(q3)])
        assert np.array_equal(quantise(p[1]), [list(q3)])
        got = decide_patchwise_host(p, Decision.from_q({1: T}, low={1: L}, min_confidence={1: 20000}))
        assert got.tolist() == [[1, 1, 1]] if kept else not got.any(), q3
    # the filter alone (L = T): a patch is judged by its mean
    p = hc.probs_of_q([[T, T, 0, 50000, 50000]])
    assert decide_patchwise_host(p, Decision.from_q({1: T}, min_confidence={1: 50000})).tolist() == [[0, 0, 0, 1, 1]]


def test_out_of_range_probabilities_follow_the_q_rule():
    p1 = np.array([[np.nan, 0.4, 1.5, -0.5, 0.4, 0.4, np.inf, -np.inf]], dtype=np.float32)
    p = np.stack([np.zeros_like(p1), p1])
    assert quantise(p1).tolist() == [[0, 26214, 65535, 0, 26214, 26214, 65535, 0]]
    dec = Decision.from_q({1: 65535}, low={1: 20000})
    assert decide_patchwise_host(p, dec).tolist() == [[0, 1, 1, 0, 1, 1, 1, 0]]
    assert decide_patchwise_host(p[:, :, :6], dec).tolist() == [[0, 1, 1, 0, 0, 0]]
    assert np.array_equal(_flood_rule(p, dec), decide_patchwise_host(p, dec))


def test_argument_errors_of_the_host_functions():
    p = hc.field(2, 37, 53)
    with pytest.raises(ValueError, match=r"\[K, h, w\]"):
        decide_patchwise_host(p[:, 0], Decision({1: .5}))
    with pytest.raises(ValueError, match="K=2"):
        decide_patchwise_host(p, Decision({1: .5, 2: .5}))
    cand = decide_host(p, Decision({1: .5}))
    labels = label_patches_host(cand, 2)
    with pytest.raises(ValueError, match="int32 label plane"):
        patch_support_host(p, cand, labels.astype(np.int64))
    with pytest.raises(ValueError, match="int32 label plane"):
        patch_support_host(p, cand[:-1], labels)
    empty = patch_support_host(p, np.zeros_like(cand), np.zeros_like(labels))
    assert all(a.size == 0 for a in empty) and empty[3].dtype == np.int64


# ---------------------------------------------------------------------- the properties of the contract on random fields
FIELDS = [(K, h, w, conn) for K in (2, 3) for h, w in hc.FIELD_SHAPES for conn in (8, 4)]


@pytest.mark.parametrize("K,h,w,conn", FIELDS)
def test_properties_on_random_fields(K, h, w, conn):
    p = hc.field(K, h, w)
    classes = range(1, K)
    plain_T = Decision.from_q({c: hc.HIGH for c in classes})
    plain_L = Decision.from_q({c: hc.LOW for c in classes})
    at_T, at_L = decide_host(p, plain_T), decide_host(p, plain_L)
    labels_L = label_patches_host(at_L, K, conn)
    for with_mean in (False, True):
        dec = hc.decision(K, conn, with_mean)
        hc.assert_not_degenerate(p, dec)
        got = decide_patchwise_host(p, dec)
        assert np.array_equal(got, _flood_rule(p, dec))
        # a patch of the candidates goes or stays whole: relabelling gives the kept patches with their roots
        assert np.array_equal(label_patches_host(got, K, conn), np.where(got > 0, labels_L, 0))
        assert np.array_equal(got[got > 0], at_L[got > 0])
        # the support rows are those of the label plane, in ascending root
        roots, cls, qmax, qsum, area = patch_support_host(p, at_L, labels_L)
        assert np.array_equal(roots, np.unique(labels_L[labels_L > 0]) - 1) and np.array_equal(cls, at_L.ravel()[roots])
        assert int(area.sum()) == int((at_L > 0).sum()) and (qmax >= hc.LOW).all() and (qsum >= hc.LOW * area).all()
        if K == 2 and not with_mean:                                # decided at T  ⊆  result  ⊆  decided at L
            assert (got[at_T > 0] == 1).all() and (at_L[got > 0] == 1).all()
            assert (got > 0).sum() > (at_T > 0).sum() and (got > 0).sum() < (at_L > 0).sum()
    # L = T and no M: the pixel rule, whatever the connectivity
    assert np.array_equal(decide_patchwise_host(p, Decision.from_q(plain_T.q, low=plain_T.q, connectivity=conn)), at_T)


def test_for_three_classes_only_the_rule_holds():
    """a pixel that is class 1 at T can be a class-2 candidate at L: decided at T is no subset of the result for K > 2"""
    q = np.array([[[0, 0, 0]], [[40000, 40000, 0]], [[0, 45000, 0]]])        # [K, 1, 3]: q_1 and q_2
    p = (q / hc.Q).astype(np.float32)
    assert np.array_equal(quantise(p), q)
    T, L = {1: 40000, 2: 50000}, {1: 40000, 2: 45000}
    assert decide_host(p, Decision.from_q(T)).tolist() == [[1, 1, 0]]
    assert decide_patchwise_host(p, Decision.from_q(T, low=L)).tolist() == [[1, 0, 0]]
