"""``ops.patch_proximity`` (csrc/proximity.hip) against ``patch_proximity_host`` by ``array_equal``, in both modes — between two
planes and, with ``exclude_own``, within one — and ``analysis.run_device`` against ``analysis.run_host`` with the ``distances``
and ``gaps`` options.  The host function is pinned to an all-pairs brute force in tests/test_proximity_host.py.  Shapes: one
pixel; one row one pixel wider than a query window (``ops.PROXIMITY_WINDOW``); one column one pixel taller than a column
segment (``ops.PROXIMITY_SEGMENT``) and a sparse plane of more than two segments (the carried states, the second candidate
across a segment border); 37 x 53; 5 x 1031 (an odd width: no row but the first starts on a 16-byte border); the two years
on 97 x 131; 64 x 300 with the only source pixel in a corner (the longest searches); an empty source plane.  Integers only:
every comparison is exact."""
import numpy as np
import pytest
import torch

import test_analysis_gpu as tag
import test_analysis_host as th
from deadtrees_amd import ops
from deadtrees_amd.deployment.patches import PatchConfig, labelled_patches_host
from deadtrees_amd.deployment.proximity import ProximityConfig, patch_distances, patch_gaps, patch_proximity_host

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = th.K


def _maps(name):
    """(source map, query map) uint8 of the named case"""
    if name == "one pixel":
        return np.ones((1, 1), np.uint8), np.ones((1, 1), np.uint8)
    if name == "one pixel, empty source":
        return np.zeros((1, 1), np.uint8), np.ones((1, 1), np.uint8)
    if name == "row":                                            # patches on both sides of the window border
        w = ops.PROXIMITY_WINDOW + 1
        a, b = th.blobs(1, w, 3, 0.02), th.blobs(1, w, 4, 0.05)
        a[0, w - 40:] = 0
        b[0, w - 3:] = 1
        return a, b
    if name == "column":
        h = ops.PROXIMITY_SEGMENT + 1
        a, b = th.blobs(h, 1, 5, 0.05), th.blobs(h, 1, 6, 0.1)
        a[h - 30:] = 0
        a[0], b[h - 1] = 2, 1                                    # the last row's nearest source lies in the first segment
        return a, b
    if name == "tall":                                           # sparse: most states are carried over a segment or two
        h = 2 * ops.PROXIMITY_SEGMENT + 9
        return th.blobs(h, 67, 7, 0.004), th.blobs(h, 67, 8, 0.02)
    if name == "odd":
        return th.blobs(37, 53, 1, 0.1), th.blobs(37, 53, 11, 0.1)
    if name == "wide":
        return th.blobs(5, 1031, 2, 0.01), th.blobs(5, 1031, 12, 0.05)
    if name == "two years":
        return th.two_years()[:2]
    if name == "corner":
        a = np.zeros((64, 300), np.uint8)
        a[63, 299] = 1
        return a, th.blobs(64, 300, 9, 0.03)
    if name == "empty source":
        return np.zeros((37, 53), np.uint8), th.blobs(37, 53, 11, 0.1)
    raise KeyError(name)


CASES = ["one pixel", "one pixel, empty source", "row", "column", "tall", "odd", "wide", "two years", "corner", "empty source"]
_PLANES = {}


def _planes(name):
    """the label planes and tables of a case, computed once: ``(ls, ts, lq, tq)``; 4-connected queries for variety"""
    if name not in _PLANES:
        a, b = _maps(name)
        (_, ls, ts), (_, lq, tq) = labelled_patches_host(a, K, PatchConfig(8)), labelled_patches_host(b, K, PatchConfig(4))
        for plane in (ls, lq):
            plane.setflags(write=False)
        _PLANES[name] = ls, ts, lq, tq
    return _PLANES[name]


def _check(ls, lq, roots, exclude_own=False, limit2=None, src=None, qry=None):
    """the device's result for the planes (uploaded here, or given as tensors) equals the host's; returns it"""
    want = patch_proximity_host(ls, lq, roots, exclude_own, limit2)
    src = torch.from_numpy(ls.copy()).to(DEV) if src is None else src
    qry = (src if ls is lq else torch.from_numpy(lq.copy()).to(DEV)) if qry is None else qry
    got = ops.patch_proximity(src, qry, roots, exclude_own, limit2)
    assert all(isinstance(g, np.ndarray) and g.dtype == np.int64 and g.shape == (len(roots),) for g in got)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (exclude_own, limit2)
    assert np.array_equal(src.cpu().numpy(), ls) and np.array_equal(qry.cpu().numpy(), lq)       # neither input is written
    return got


@pytest.mark.parametrize("name", CASES)
def test_device_equals_host_in_both_modes(name):
    ls, ts, lq, tq = _planes(name)
    d2, _ = _check(ls, lq, tq.root)
    _check(lq, ls, ts.root)                                      # the other direction
    gap, _ = _check(lq, lq, tq.root, True)
    _check(ls, ls, ts.root, True)
    if name in ("one pixel, empty source", "empty source"):
        assert tq.n > 0 and (d2 == -1).all()
    elif name == "corner":
        assert ts.n == 1 and tq.n > 50 and d2.min() > 0 and d2.max() > 250 ** 2
    elif name != "one pixel":
        assert tq.n > 1 and d2.max() > 0 and (gap > 0).any()     # worth comparing


def test_crossing_shapes_cross():
    S, W = ops.PROXIMITY_SEGMENT, ops.PROXIMITY_WINDOW
    assert _planes("row")[0].shape == (1, W + 1) and _planes("column")[0].shape == (S + 1, 1)
    ls, ts, lq, tq = _planes("row")
    assert lq[0, W] > 0 and lq[0, W] == lq[0, W - 1]             # a query patch across the window border
    d2, _ = patch_proximity_host(ls, lq, tq.root)
    assert d2[-1] > 30 ** 2                                      # whose search goes far into the first window
    ls, ts, lq, tq = _planes("column")
    d2, near = patch_proximity_host(ls, lq, tq.root)
    assert d2[-1] >= 29 ** 2 and ls[:S].any() and not ls[S:].any()   # the last segment's answers are all carried in
    ls = _planes("tall")[0]
    assert ls.shape[0] > 2 * S and (ls.any(axis=1).reshape(-1)[:S].any())


@pytest.mark.parametrize("exclude_own", [False, True])
def test_limits(exclude_own):
    ls, ts, lq, tq = _planes("two years")
    src = lq if exclude_own else ls
    free, _ = _check(src, lq, tq.root, exclude_own)
    at_zero, _ = _check(src, lq, tq.root, exclude_own, 0)
    cut, _ = _check(src, lq, tq.root, exclude_own, 9)
    beyond, _ = _check(src, lq, tq.root, exclude_own, 97 ** 2 + 131 ** 2)
    assert np.array_equal(beyond, free) and np.array_equal(at_zero, np.where(free == 0, 0, -1))
    assert np.array_equal(cut, np.where(free <= 9, free, -1)) and 0 < (cut < 0).sum() < tq.n
    exact = int(free[free > 0].max())                            # a pair at exactly the limit counts, one below does not
    assert (_check(src, lq, tq.root, exclude_own, exact)[0] == exact).any()
    assert not (_check(src, lq, tq.root, exclude_own, exact - 1)[0] == exact).any()


def test_views_offsets_and_root_arguments():
    ls, ts, lq, tq = _planes("odd")
    h, w = ls.shape
    # a non-contiguous view, and a plane at an odd storage offset
    wide = torch.zeros((h, 2 * w), dtype=torch.int32, device=DEV)
    wide[:, ::2] = torch.from_numpy(ls.copy()).to(DEV)
    flat = torch.zeros(h * w + 1, dtype=torch.int32, device=DEV)
    flat[1:] = torch.from_numpy(lq.copy()).to(DEV).view(-1)
    src, qry = wide[:, ::2], flat[1:].view(h, w)
    assert not src.is_contiguous() and qry.data_ptr() % 16 == 4
    _check(ls, lq, tq.root, src=src, qry=qry)
    _check(lq, lq, tq.root, True, src=qry, qry=qry)
    # the roots as a device tensor; a subset of the table; no roots at all
    want = patch_proximity_host(ls, lq, tq.root)
    got = ops.patch_proximity(src, qry, torch.from_numpy(tq.root.copy()).to(DEV))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    _check(ls, lq, tq.root[::3].copy())
    none = ops.patch_proximity(src, qry, np.zeros(0, np.int64))
    assert none[0].shape == none[1].shape == (0,) and none[0].dtype == none[1].dtype == np.int64
    for bad, fragment in (((src.long(), qry, tq.root), "int32"), ((src[:-1], qry, tq.root), "int32"),
                          ((src, qry, tq.root, False, -1), "limit2"), ((src, qry, tq.root.astype(np.float32)), "roots_qry")):
        with pytest.raises(RuntimeError, match=fragment):
            ops.patch_proximity(*bad)


# ---------------------------------------------------------------------------------------------- the device runner
@pytest.mark.parametrize("config", tag.CONFIGS, ids=repr)
@pytest.mark.parametrize("against_as", ["array", "polygons"])
def test_run_device_equals_run_host(config, against_as):
    a, b, zones = th.two_years()
    if against_as == "polygons":
        a = tag._squares(97, 131, (1, 2), 25, 7)
    base = dict(zones=zones, patches=config, outlines=True, against=a, against_patches=tag.AGAINST_CONFIG)
    plain_map, plain = tag._both(b, **base)
    limit = ProximityConfig(2)
    _, apart = tag._both(b, distances=True, **base)
    _, gaps = tag._both(b, gaps=limit, **{k: v for k, v in base.items() if k not in ("against", "against_patches")})
    full_map, full = tag._both(b, distances=limit, gaps=True, **base)
    # worth comparing: patches that touch the other map, patches apart, patches without a neighbour within the limit
    far = apart.overlaps.distances
    assert (far.b_d2 == 0).any() and (far.b_d2 > 0).any() and (far.a_d2 > 0).any() and (far.b_d2 >= 0).all()
    assert (gaps.gaps.d2 < 0).any() and (gaps.gaps.d2 > 0).any() and gaps.overlaps is None
    assert (np.concatenate([full.overlaps.distances.a_d2, full.overlaps.distances.b_d2]) < 0).any() and (full.gaps.d2 > 0).all()
    assert np.array_equal(far.b_d2 == 0, full.overlaps.partners_b() > 0)
    # everything else is what the call without the options returns
    for other in (apart, full):
        assert np.array_equal(full_map, plain_map) and other.patches == plain.patches and other != plain
        assert np.array_equal(other.counts, plain.counts) and np.array_equal(other.outlines.xy, plain.outlines.xy)
        assert all(np.array_equal(getattr(other.overlaps, c), getattr(plain.overlaps, c)) for c in "abn")
        assert other.overlaps.table_a == plain.overlaps.table_a
    assert gaps.patches == plain.patches and plain.gaps is None and plain.overlaps.distances is None


def test_maps_in_on_the_device():
    a, b, _ = th.two_years()
    limit = ProximityConfig(5)
    want = patch_distances(a, b, K, PatchConfig(8, 3), PatchConfig(4, 6), limit)
    assert patch_distances(a, b, K, PatchConfig(8, 3), PatchConfig(4, 6), limit, device=DEV) == want
    assert patch_distances(torch.from_numpy(a).to(DEV), b, K, PatchConfig(8, 3), PatchConfig(4, 6), limit) == want
    assert patch_gaps(torch.from_numpy(b).to(DEV), K, PatchConfig(4, 6)) == patch_gaps(b, K, PatchConfig(4, 6))
    polys = tag._squares(97, 131, (1, 2), 25, 7)
    assert patch_distances(polys, b, K, device=DEV) == patch_distances(polys, b, K)
