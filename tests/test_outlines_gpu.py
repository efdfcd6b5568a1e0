"""Dead-tree patch outlines on the device: ``csrc/outlines.hip`` through ``ops.patch_outlines`` against ``polygonize_host``
(itself pinned to a scalar wall follower in tests/test_outlines_host.py), the round trip through the device rasteriser, and
``infer_tile`` / ``infer_rasters`` with ``outlines=True`` on every device path.  Integers only: every comparison is
``array_equal`` on the four ``PolygonSet`` arrays.

Maps: the patterns and shapes of tests/test_patches_gpu.py (its ``_map``, ``_shapes`` and ``PATTERNS``, imported unchanged),
plus single rows of ``C - 1``, ``C`` and ``C + 1`` pixels and three rows of ``C`` for ``C = ops.OUTLINE_CHUNK``: a chunk
boundary of the compaction inside a row and at a row start.  The spiral and the serpentine at (257, 300) are ONE ring of tens
of thousands of edges — every pointer-jumping round, across many workgroups; the 8-connected checkerboard has the most
edges.  No map exceeds 300 x 470 or 140,000 pixels."""
import functools

import numpy as np
import pytest
import torch

import test_patches_gpu as tp
from test_patches_gpu import ckpts, ensemble, inf  # noqa: F401  (module-scoped fixtures: three checkpoints, their ensemble)

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = 3
CONNECTIVITIES = (4, 8)


def _shapes():
    from deadtrees_amd import ops
    C = ops.OUTLINE_CHUNK
    extra = [(1, C - 1), (1, C), (1, C + 1), (3, C)]
    assert all(h * w < 140_000 for h, w in extra)
    return tp._shapes() + extra


def _arrays(p):
    return p.xy, p.ring_offsets, p.ring_polygon, p.values


def _same(got, want, what=None):
    for name, x, y in zip(("xy", "ring_offsets", "ring_polygon", "values"), _arrays(got), _arrays(want)):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), (name, what)


@functools.lru_cache(maxsize=None)
def _host(pattern, h, w, connectivity):
    """(labels, outlines) of the host contract, computed once"""
    from deadtrees_amd.deployment.outlines import polygonize_host
    from deadtrees_amd.deployment.patches import label_patches_host
    c = tp._map(pattern, h, w)
    labels = label_patches_host(c, K, connectivity)
    labels.setflags(write=False)
    return labels, polygonize_host(c, K, connectivity, labels=labels)


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


# ---------------------------------------------------------------------------------------------- 1. against the host
@pytest.mark.parametrize("pattern", tp.PATTERNS)
def test_patch_outlines_against_the_host(pattern):
    from deadtrees_amd import ops
    for h, w in _shapes():
        for conn in CONNECTIVITIES:
            c = tp._map(pattern, h, w)
            host_labels, want = _host(pattern, h, w, conn)
            dc = _dev(c)
            labels, err = ops.label_patches(dc, K, conn)
            assert int(err) == 0 and np.array_equal(labels.cpu().numpy(), host_labels)
            keep = labels.clone()
            got = ops.patch_outlines(labels, dc, conn)
            _same(got, want, (pattern, h, w, conn))
            assert torch.equal(labels, keep) and np.array_equal(dc.cpu().numpy(), c)      # nothing wrote to either plane
            assert len(got) == ops.patch_table(labels, dc).n
            if pattern == "background":
                assert len(got) == 0 and len(got.xy) == 0
            elif pattern == "all one":
                assert got.xy.tolist() == [[256 * w, 0], [256 * w, 256 * h], [0, 256 * h], [0, 0]]
            elif pattern in ("spiral", "serpentine") and (h, w) == (257, 300):
                assert len(got) == 1 and len(got.ring_polygon) == 1                      # one long ring
                assert int(np.count_nonzero(host_labels)) > 30_000
            elif pattern == "checkerboard 0/1" and conn == 8 and min(h, w) > 1:
                assert len(got) == 1 and len(got.xy) == 4 * ((h * w) // 2)               # every side of every pixel turns


def test_the_label_plane_of_a_sieved_map():
    from deadtrees_amd import ops
    from deadtrees_amd.deployment.outlines import polygonize_host
    for conn in CONNECTIVITIES:
        dc = _dev(tp._map("random 0.59", 257, 300))
        labels, _ = ops.label_patches(dc, K, conn)
        area = ops.patch_areas(labels)
        ops.sieve_patches(dc, labels, area, 5)
        got = ops.patch_outlines(labels, dc, conn)
        sieved = dc.cpu().numpy()
        assert not np.array_equal(sieved, tp._map("random 0.59", 257, 300))
        _same(got, polygonize_host(sieved, K, conn), conn)
        table = ops.patch_table(labels, dc, area)
        assert len(got) == table.n and np.array_equal(got.values, table.cls)


# ---------------------------------------------------------------------------------------------- 2. views, repetition
def test_views_with_a_storage_offset_and_non_contiguous_slices():
    from deadtrees_amd import ops
    from deadtrees_amd.deployment.outlines import polygonize_host
    big = tp._map("random 0.59", 257, 300)
    dbig = _dev(big)
    crop = (slice(7, 251), slice(3, 290, 2))                                     # non-contiguous: made contiguous
    sub = np.ascontiguousarray(big[crop])
    labels, _ = ops.label_patches(dbig[crop], K)
    assert not dbig[crop].is_contiguous()
    _same(ops.patch_outlines(labels, dbig[crop]), polygonize_host(sub, K))
    rows = (slice(40, 140), slice(None))                                         # labels as a non-contiguous view, too
    part_labels, _ = ops.label_patches(dbig[rows], K)
    padded = torch.zeros((100, 310), dtype=torch.int32, device=DEV)
    padded[:, 5:305] = part_labels
    assert not padded[:, 5:305].is_contiguous()
    _same(ops.patch_outlines(padded[:, 5:305], dbig[rows]), polygonize_host(np.ascontiguousarray(big[rows]), K))
    assert dbig[rows].is_contiguous() and dbig[rows].storage_offset() == 40 * 300
    # member m of a stacked [M, h, w] tensor with odd h * w: contiguous views at odd byte offsets
    stack = np.stack([tp._map(p, 37, 53) for p in ("random 0.59", "random 0.03", "spiral")])
    ds = _dev(stack)
    all_labels = torch.stack([ops.label_patches(ds[m], K, 4)[0] for m in range(3)])
    for m in range(3):
        assert ds[m].is_contiguous() and all_labels[m].storage_offset() == m * 37 * 53
        _same(ops.patch_outlines(all_labels[m], ds[m], 4), polygonize_host(stack[m], K, 4), m)
    assert np.array_equal(ds.cpu().numpy(), stack) and np.array_equal(dbig.cpu().numpy(), big)


def test_the_same_call_twice_gives_identical_arrays():
    from deadtrees_amd import ops
    for pattern in ("random 0.59", "spiral"):
        dc = _dev(tp._map(pattern, 257, 300))
        labels, _ = ops.label_patches(dc, K)
        first = ops.patch_outlines(labels, dc)
        second = ops.patch_outlines(labels, dc)
        _same(first, second, pattern)
        _same(first, _host(pattern, 257, 300, 8)[1], pattern)


def test_argument_errors_are_raised_on_the_host():
    from deadtrees_amd import _lib, ops
    dc = _dev(tp._map("random 0.03", 97, 131))
    labels, _ = ops.label_patches(dc, K)
    for conn in (0, 6, True, "8"):
        with pytest.raises(RuntimeError):
            ops.patch_outlines(labels, dc, conn)
    with pytest.raises(RuntimeError):
        ops.patch_outlines(labels.long(), dc)
    with pytest.raises(RuntimeError):
        ops.patch_outlines(labels, dc.int())
    with pytest.raises(RuntimeError):
        ops.patch_outlines(labels[:, :-1], dc)
    with pytest.raises(RuntimeError):
        ops.patch_outlines(labels.view(-1), dc.view(-1))
    with pytest.raises(RuntimeError):
        ops.patch_outlines(labels.cpu(), dc)
    with pytest.raises(RuntimeError):
        ops.patch_outlines(labels, dc.cpu())
    # the entry points refuse a raster beyond the key range before any launch
    lib = _lib.load()
    counts = torch.zeros((4, 2), dtype=torch.int32, device=DEV)
    assert lib.dt_outline_count(labels.data_ptr(), 16385, 1, counts.data_ptr(), _lib.stream()) != 0
    assert lib.dt_outline_count(labels.data_ptr(), 70000, 70000, counts.data_ptr(), _lib.stream()) != 0
    assert lib.dt_outline_count(labels.data_ptr(), 0, 5, counts.data_ptr(), _lib.stream()) != 0
    assert b"1..16384" in lib.dt_last_error()
    assert not counts.any()
    assert isinstance(ops.OUTLINE_CHUNK, int) and ops.OUTLINE_CHUNK % 256 == 0
    _same(ops.patch_outlines(labels, dc), _host("random 0.03", 97, 131, 8)[1])          # and nothing was left behind


# ---------------------------------------------------------------------------------------------- 3. the round trip
@pytest.mark.parametrize("pattern", ["random 0.59", "checkerboard 1/2", "spiral", "comb"])
def test_round_trip_through_the_device_rasteriser(pattern):
    from deadtrees_amd import ops
    from deadtrees_amd.deployment.outlines import polygonize
    for h, w in ((97, 131), (257, 300)):
        for conn in CONNECTIVITIES:
            c = tp._map(pattern, h, w)
            dc = _dev(c)
            labels, _ = ops.label_patches(dc, K, conn)
            polys = ops.patch_outlines(labels, dc, conn)
            edges, table = polys.tables()
            back = ops.rasterize_polygons(torch.from_numpy(edges.copy()).to(DEV), torch.from_numpy(table.copy()).to(DEV),
                                          (h, w), all_touched=False)
            assert np.array_equal(back.cpu().numpy(), c), (h, w, conn)
            _same(polygonize(dc, K, conn), polys)                               # the public entry takes the device path
            _same(polygonize(c, K, conn, device=DEV), polys)


# ---------------------------------------------------------------------------------------------- 4. end to end
@pytest.mark.parametrize("min_pixels", [0, 4])
@pytest.mark.parametrize("case", list(tp.E2E))
def test_infer_tile_outlines_on_every_path(inf, ensemble, case, min_pixels):
    from deadtrees_amd.deployment.outlines import polygonize_host
    from deadtrees_amd.deployment.patches import PatchConfig
    from deadtrees_amd.deployment.tiler import infer_tile
    raster = tp._raster(tp.H, tp.W, 31)
    model = ensemble if "vote" in case else inf
    kw = dict(subtile=tp.D, batch_size=16, device=DEV, stats=True, **tp.E2E[case])
    if case == "soft vote":
        ensemble.vote = "soft"
    try:
        for config in (PatchConfig(8, min_pixels), PatchConfig(4, min_pixels)):
            without = infer_tile(model, raster, patches=config, **kw)
            got = infer_tile(model, raster, patches=config, outlines=True, **kw)
            assert len(got) == len(without) and without[-1].outlines is None
            assert got[0].dtype == np.uint8 and np.array_equal(got[0], without[0])
            if case == "average+probs":
                assert np.array_equal(got[1], without[1])
            assert got[-1].patches == without[-1].patches and np.array_equal(got[-1].counts, without[-1].counts)
            _same(got[-1].outlines, polygonize_host(got[0], 2, config.connectivity), (case, config))
            assert len(got[-1].outlines) == got[-1].patches.n
            assert np.array_equal(got[-1].outlines.values, got[-1].patches.cls)
            if model is inf:
                assert got[-1].patches.n > 50                                    # a map worth tracing
    finally:
        ensemble.vote = "hard"


def test_infer_rasters_passes_outlines_through_and_outlines_need_patches(inf):
    from deadtrees_amd.deployment.outlines import polygonize_host
    from deadtrees_amd.deployment.patches import PatchConfig
    from deadtrees_amd.deployment.tiler import infer_rasters, infer_tile
    queue = [("a", tp._raster(130, 77, 43)), ("b", tp._raster(64, 200, 47))]
    kw = dict(subtile=tp.D, batch_size=16, device=DEV, overlap=16, blend="crop")
    plain = dict(infer_rasters(inf, queue, stats=True, patches=PatchConfig(8, 3), **kw))
    got = dict(infer_rasters(inf, queue, stats=True, patches=PatchConfig(8, 3), outlines=True, **kw))
    for key in ("a", "b"):
        assert np.array_equal(got[key][0], plain[key][0]) and got[key][1].patches == plain[key][1].patches
        _same(got[key][1].outlines, polygonize_host(got[key][0], 2, 8), key)
        assert plain[key][1].outlines is None
    assert (got["a"][1] + got["b"][1]).outlines is None
    with pytest.raises(ValueError):
        next(infer_rasters(inf, queue, stats=True, outlines=True, **kw))
    with pytest.raises(ValueError):
        infer_tile(inf, queue[0][1], stats=True, outlines=True, **kw)
    with pytest.raises(ValueError):
        infer_tile(inf, queue[0][1], stats=True, patches=True, outlines="yes", **kw)
