"""The patch-wise decision on the device (``csrc/curves.hip`` through ``ops.decide_patchwise``) against the host rule of
``loss/curves.py`` with ``array_equal`` — everything is an integer.  The support pass is compared apart from the rejection
(``return_support=True`` against ``patch_support_host``), and ``infer_tile`` with a patch-wise decision against the host
functions on the probabilities it returns.

Shapes: the random fields of tests/hysteresis_cases.py (several workgroups of every launch; 131 x 257 and 37 x 53 have an
odd pixel count, so the scalar tail and unaligned class planes run), one patch over a whole plane (the carry across
chunks, waves and workgroups and many writers on one root), a sum past 2^32, a checkerboard of single-pixel patches, runs
that end or wrap at a row end, and K = 8."""
import numpy as np
import pytest
import torch

import hysteresis_cases as hc
from deadtrees_amd import ops
from deadtrees_amd.deployment.patches import label_patches_host
from deadtrees_amd.loss.curves import Decision, decide_host, decide_patchwise_host, patch_support_host, quantise

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)        # (a copy: the shared fields are read-only)


def _low_decision(dec, K):
    return Decision.from_q({c: int(dec.low_u16(K)[c]) for c in range(1, K)})


def _check(p, dec, want=None):
    """``ops.decide_patchwise`` on ``p``: the map against the host rule (or ``want``), the label plane and the support
    planes against the host's — the roots' entries, 0 elsewhere —, and ``out=`` written in place"""
    K, h, w = p.shape
    want = decide_patchwise_host(p, dec) if want is None else want
    cand = decide_host(p, _low_decision(dec, K))
    labels = label_patches_host(cand, K, dec.connectivity)
    roots, _, qmax, qsum, area = patch_support_host(p, cand, labels)
    got, got_labels, got_qmax, got_qsum, got_area = ops.decide_patchwise(_dev(p), dec, return_support=True)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (h, w)
    assert got_labels.dtype == torch.int32 and np.array_equal(got_labels.cpu().numpy(), labels)
    planes = [(got_qmax, torch.int32, qmax)]
    if dec.min_confidence:
        planes += [(got_qsum, torch.int64, qsum), (got_area, torch.int32, area)]
    else:
        assert got_qsum is None and got_area is None
    for plane, dtype, values in planes:
        full = np.zeros(h * w, np.int64)
        full[roots] = values
        assert plane.dtype == dtype and tuple(plane.shape) == (h * w,)
        assert np.array_equal(plane.cpu().numpy().astype(np.int64), full)
    assert np.array_equal(got.cpu().numpy(), want)
    out = torch.full((h, w), 255, dtype=torch.uint8, device=DEV)
    assert ops.decide_patchwise(_dev(p), dec, out=out) is out and np.array_equal(out.cpu().numpy(), want)
    return want


FIELDS = [(K, h, w) for K in (2, 3) for h, w in hc.FIELD_SHAPES + ((37, 53),)]


@pytest.mark.parametrize("with_mean", [False, True], ids=["no M", "M"])
@pytest.mark.parametrize("conn", [8, 4])
@pytest.mark.parametrize("K,h,w", FIELDS)
def test_fields_equal_the_host(K, h, w, conn, with_mean):
    p = hc.field(K, h, w)
    dec = hc.decision(K, conn, with_mean)
    if (h, w) in hc.FIELD_SHAPES:                                  # 37 x 53 is a shape case only
        hc.assert_not_degenerate(p, dec)
    else:
        assert (h * w) % 4 != 0 and h * w > 1024
    want = _check(p, dec)
    assert want.any()
    # a view that starts off the 16-byte grid
    flat = _dev(np.concatenate([np.zeros(3, dtype=np.float32), p.reshape(-1)]))[3:].view(K, h, w)
    assert np.array_equal(ops.decide_patchwise(flat, dec).cpu().numpy(), want)


@pytest.mark.parametrize("K", [2, 3])
def test_a_decision_that_is_not_patchwise_equals_decide_classes(K):
    p = hc.field(K, 37, 53)
    for conn in (8, 4):
        dec = Decision.from_q({c: hc.HIGH for c in range(1, K)}, low={c: hc.HIGH for c in range(1, K)}, connectivity=conn)
        assert not dec.patchwise
        plain = ops.decide_classes(_dev(p), dec)
        assert torch.equal(ops.decide_patchwise(_dev(p), dec), plain)
        # with the support asked for, the four launches run and give the same map: every candidate is its own proof
        assert torch.equal(ops.decide_patchwise(_dev(p), dec, return_support=True)[0], plain)
        assert np.array_equal(plain.cpu().numpy(), decide_host(p, dec))


def test_out_of_range_probabilities():
    p1 = np.array([[np.nan, 0.4, 1.5, -0.5, 0.4, 0.4, np.inf, -np.inf]], dtype=np.float32)
    p = np.stack([np.zeros_like(p1), p1])
    dec = Decision.from_q({1: 65535}, low={1: 20000})
    assert _check(p, dec).tolist() == [[0, 1, 1, 0, 1, 1, 1, 0]]
    assert _check(np.ascontiguousarray(p[:, :, :6]), dec).tolist() == [[0, 1, 1, 0, 0, 0]]


@pytest.mark.parametrize("mean", [None, hc.LOW], ids=["no M", "M"])
def test_one_patch_over_the_whole_plane(mean):
    """131 x 257 at q = L: the LAST pixel decides.  Every run is carried through its wave's chunks, and every workgroup
    writes to root 0"""
    h, w = 131, 257
    assert h * w > 8 * 4 * ops.SUPPORT_SPAN * 64                   # more than eight workgroups of the support pass
    dec = Decision.from_q({1: hc.HIGH}, low={1: hc.LOW}, min_confidence=None if mean is None else {1: mean})
    for last, kept in ((hc.HIGH, True), (hc.HIGH - 1, False)):
        q = np.full((h, w), hc.LOW, np.int64)
        q[-1, -1] = last
        p = hc.probs_of_q(q)
        assert np.array_equal(quantise(p[1]), q)
        want = _check(p, dec, np.full((h, w), int(kept), np.uint8))
        assert np.array_equal(want, decide_patchwise_host(p, dec))


def test_a_sum_past_32_bits():
    """259 x 257 at q = 65535 with M = 65535: S = 65535 * 66563 > 2^32 equals M * A; one pixel at 65534 and S = M * A - 1"""
    h, w = 259, 257
    assert hc.Q * h * w > 2 ** 32
    dec = Decision.from_q({1: hc.Q}, low={1: 60000}, min_confidence={1: hc.Q})
    for dent, kept in ((None, True), ((100, 77), False)):
        q = np.full((h, w), hc.Q, np.int64)
        if dent:
            q[dent] = hc.Q - 1
        p = hc.probs_of_q(q)
        assert np.array_equal(quantise(p[1]), q)
        want = _check(p, dec, np.full((h, w), int(kept), np.uint8))
        assert np.array_equal(want, decide_patchwise_host(p, dec))


def test_a_checkerboard_of_single_pixel_patches():
    h, w = 64, 66
    y, x = np.mgrid[:h, :w]
    board, strong = (y + x) % 2 == 0, (y * w + x) % 3 == 0
    q = np.where(board, np.where(strong, hc.HIGH, hc.HIGH - 1), 0)
    p = hc.probs_of_q(q)
    assert np.array_equal(quantise(p[1]), q)
    for mean in (None, hc.HIGH):                                    # a single pixel at T - 1 fails either test
        conf = None if mean is None else {1: mean}
        four = Decision.from_q({1: hc.HIGH}, low={1: hc.LOW}, min_confidence=conf, connectivity=4)
        assert np.array_equal(_check(p, four), (board & strong).astype(np.uint8))
    eight = Decision.from_q({1: hc.HIGH}, low={1: hc.LOW}, connectivity=8)
    assert np.array_equal(_check(p, eight), board.astype(np.uint8))                   # one patch, kept whole
    # its mean lies between T - 1 and T: the filter at T rejects it whole
    eight_mean = Decision.from_q({1: hc.HIGH}, low={1: hc.LOW}, min_confidence={1: hc.HIGH}, connectivity=8)
    assert not _check(p, eight_mean).any()


def test_runs_that_end_or_wrap_at_a_row_end():
    """40 x 53.  P1 ends row 3 and P2 begins row 4: consecutive pixels of the row-major walk, two patches, and only P1 holds a
    pixel at T.  U is U-shaped: the end of row 20 and the beginning of row 21 belong to it (they meet through row 22), so one
    run of equal labels wraps the row end; its only strong pixel lies behind the wrap"""
    h, w = 40, 53
    q = np.zeros((h, w), np.int64)
    q[3, w - 3:] = hc.LOW
    q[3, w - 1] = hc.HIGH                                           # P1
    q[4, :3] = hc.HIGH - 1                                          # P2: no pixel at T
    q[20, w - 2:] = hc.LOW
    q[21, :2] = hc.LOW
    q[21, w - 1] = hc.LOW
    q[22, :] = hc.LOW
    q[21, 1] = hc.HIGH                                              # U
    q[30, 10:20] = hc.HIGH - 1                                      # a patch inside a row, rejected
    p = hc.probs_of_q(q)
    assert np.array_equal(quantise(p[1]), q)
    want = (q > 0).astype(np.uint8)
    want[4, :3] = 0
    want[30] = 0
    for conn in (8, 4):
        cand = (q > 0).astype(np.uint8)
        labels = label_patches_host(cand, 2, conn)
        assert labels[3, w - 1] != labels[4, 0] and labels[20, w - 1] == labels[21, 0] == 20 * w + w - 2 + 1
        assert np.array_equal(_check(p, Decision.from_q({1: hc.HIGH}, low={1: hc.LOW}, connectivity=conn)), want)
        # with the filter at the mean of U (its sum over its area, rounded down): kept at the boundary, rejected above it
        roots, _, _, qsum, area = patch_support_host(p, cand, labels)
        u = int(np.flatnonzero(roots == 20 * w + w - 2)[0])
        mean = int(qsum[u] // area[u])
        at = Decision.from_q({1: hc.HIGH}, low={1: hc.LOW}, min_confidence={1: mean}, connectivity=conn)
        above = Decision.from_q({1: hc.HIGH}, low={1: hc.LOW}, min_confidence={1: mean + 1}, connectivity=conn)
        assert _check(p, at)[22].all() and not _check(p, above)[22].any()


def test_eight_classes():
    K, h, w = 8, 33, 47
    p = hc.field(K, h, w)
    for conn in (8, 4):
        for with_mean in (False, True):
            dec = hc.decision(K, conn, with_mean)
            want = _check(p, dec)
            cand = decide_host(p, _low_decision(dec, K))
            assert len(np.unique(want)) >= 5 and (want != cand).any()       # several classes survive, something is rejected


def test_argument_errors():
    p = _dev(hc.field(2, 37, 53))
    dec = hc.decision(2, 8, True)
    with pytest.raises(RuntimeError, match=r"\[K, h, w\]"):
        ops.decide_patchwise(p[1], dec)
    with pytest.raises(RuntimeError, match=r"\[K, h, w\]"):
        ops.decide_patchwise(p.view(2, 1, 37, 53), dec)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.decide_patchwise(p[:, :, ::2], dec)
    with pytest.raises(RuntimeError, match="float32"):
        ops.decide_patchwise(p.double(), dec)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.decide_patchwise(p.cpu(), dec)
    for out in (torch.zeros((37, 54), dtype=torch.uint8, device=DEV), torch.zeros((37, 53), dtype=torch.int32, device=DEV),
                torch.zeros((37, 106), dtype=torch.uint8, device=DEV)[:, ::2]):
        with pytest.raises(RuntimeError, match="out must be"):
            ops.decide_patchwise(p, dec, out=out)
    with pytest.raises(ValueError, match="K=2"):
        ops.decide_patchwise(p, hc.decision(3, 8, True))
    with pytest.raises(ValueError, match="must be a Decision"):
        ops.decide_patchwise(p, [0, 30000])
    assert isinstance(ops.SUPPORT_SPAN, int) and ops.SUPPORT_SPAN >= 1


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


def _a_decision_that_keeps_and_rejects(probs, connectivity):
    """L and T from quantiles of q_1, chosen on the host so that the rule keeps at least one patch and rejects at least one"""
    q1 = quantise(probs[1])
    for low_share, high_share in ((0.5, 0.9), (0.6, 0.95), (0.7, 0.98), (0.4, 0.8), (0.8, 0.99), (0.3, 0.7), (0.9, 0.999)):
        L, T = max(1, int(np.quantile(q1, low_share))), max(1, int(np.quantile(q1, high_share)))
        if L >= T:
            continue
        dec = Decision.from_q({1: T}, low={1: L}, connectivity=connectivity)
        _, core, _ = hc.patch_fates(probs, dec)
        if core.any() and not core.all():
            return dec
    raise AssertionError("no pair of quantiles keeps one patch and rejects another")


def test_infer_tile_with_a_patchwise_decision(inference, monkeypatch):
    from deadtrees_amd.deployment.attributes import AttributeConfig, patch_attributes_host
    from deadtrees_amd.deployment.patches import PatchConfig, labelled_patches_host
    from deadtrees_amd.deployment.tiler import infer_rasters, infer_tile
    raster = np.random.default_rng(31).integers(0, 256, (3, 200, 232), dtype=np.uint8)
    kw = dict(subtile=128, overlap=64, blend="average", device=DEV, batch_size=4)
    plain_map, probs = infer_tile(inference, raster, return_probs=True, **kw)
    for connectivity in (8, 4):
        decision = _a_decision_that_keeps_and_rejects(probs, connectivity)
        _, core, _ = hc.patch_fates(probs, decision)
        assert core.any() and not core.all()
        want = decide_patchwise_host(probs, decision)
        assert want.any() and (want != decide_host(probs, _low_decision(decision, 2))).any()
        got = infer_tile(inference, raster, decision=decision, **kw)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)       # no probabilities
        got_map, got_probs = infer_tile(inference, raster, return_probs=True, decision=decision, **kw)
        assert np.array_equal(got_map, want) and np.array_equal(got_probs, probs)
        # everything downstream sees the decided map
        config, confident = PatchConfig(connectivity), AttributeConfig(confidence=True)
        st_map, st = infer_tile(inference, raster, decision=decision, stats=True, patches=config, attributes=confident, **kw)
        assert np.array_equal(st_map, want) and np.array_equal(st.counts.reshape(-1), np.bincount(want.reshape(-1), minlength=2))
        _, labels, table = labelled_patches_host(want, 2, config)
        assert st.patches == table and table.n > 0
        assert st.attributes == patch_attributes_host(labels, table, raster, want, probs, AttributeConfig(None, True))
        # with a confidence filter at the median of the kept patches' means: some kept patch goes
        cand = decide_host(probs, _low_decision(decision, 2))
        _, _, qmax, qsum, area = patch_support_host(probs, cand, label_patches_host(cand, 2, connectivity))
        kept = qmax >= decision.q[1]
        means = np.sort(qsum[kept] // area[kept])
        filtered = Decision.from_q(decision.q, low=decision.low, min_confidence={1: int(means[len(means) // 2]) + 1},
                                   connectivity=connectivity)
        want_f = decide_patchwise_host(probs, filtered)
        assert (want_f != want).any()
        assert np.array_equal(infer_tile(inference, raster, decision=filtered, **kw), want_f)
    (key, from_loop), = list(infer_rasters(inference, [("a", raster)], subtile=128, overlap=64, blend="average", device=DEV,
                                           batch_size=4, decision=decision))
    assert key == "a" and np.array_equal(from_loop, want)

    # a decision that is not patch-wise takes the plain path: ops.decide_patchwise is not called
    def never(*a, **k):
        raise AssertionError("a plain decision must not reach ops.decide_patchwise")
    monkeypatch.setattr(ops, "decide_patchwise", never)
    plain = Decision.from_q(decision.q, low=decision.q, connectivity=4)
    assert not plain.patchwise
    assert np.array_equal(infer_tile(inference, raster, decision=plain, **kw), decide_host(probs, plain))
    with pytest.raises(AssertionError, match="must not reach"):
        infer_tile(inference, raster, decision=decision, **kw)


def test_a_patchwise_decision_is_refused_where_a_plain_one_is():
    from deadtrees_amd.deployment.tiler import infer_tile

    class Stub:
        classes = 2

        def run_windows(self, *a, **k):
            raise AssertionError("nothing may run before the arguments are checked")

    class Ensemble(Stub):
        members, vote = [Stub(), Stub()], "hard"
    raster = np.zeros((3, 64, 64), dtype=np.uint8)
    d = hc.decision(2, 8, True)
    with pytest.raises(ValueError, match="infer_tile.*average"):
        infer_tile(Stub(), raster, overlap=16, blend="crop", decision=d)
    with pytest.raises(ValueError, match="soft"):
        infer_tile(Ensemble(), raster, overlap=16, blend="average", decision=d)
    with pytest.raises(ValueError, match="infer_tile"):
        infer_tile(Stub(), raster, overlap=16, blend="average", decision=hc.decision(3, 8, False))
