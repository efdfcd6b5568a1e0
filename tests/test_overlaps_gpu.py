"""Patch overlaps on the device: ``csrc/overlaps.hip`` through ``ops.patch_overlaps`` against ``overlap_pairs_host``
(itself pinned to a scalar loop and hand answers in tests/test_overlaps_host.py), ``patch_overlaps(..., device="cuda")``
against the host route, and ``infer_tile`` / ``infer_rasters`` with ``against=`` on the device paths.  Integers only: every
comparison is ``array_equal``.

The label planes of part 1 are made on the CPU (``label_patches_host``), so that the overlap kernels are tested on their
own.  Shapes: one pixel; a row and a column of 2 C + 1 pixels for C = ``ops.OVERLAP_CHUNK`` (two chunk borders); 37 x 53
(an odd pixel count: the tail of the 16-byte loads); 3 x (C + 1) (a run that wraps a row end and a chunk border at
once); a 4-connected checkerboard against one raster-sized patch (every pixel a run); patches in the last rows of 300 x
300 (roots above 2^16); random blobs at connectivity 4 against connectivity 8.  No plane exceeds 90,000 pixels."""
import numpy as np
import pytest
import torch

import test_patches_gpu as tp
from test_patches_gpu import ckpts, ensemble, inf  # noqa: F401  (module-scoped fixtures: three checkpoints, their ensemble)

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = 3


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def _labels(c, connectivity=8):
    from deadtrees_amd.deployment.patches import label_patches_host
    return label_patches_host(np.ascontiguousarray(c, dtype=np.uint8), K, connectivity)


def _blobs(h, w, seed, density=0.08):
    """seeds dilated by a 3 x 3 square, classes 1 and 2"""
    rng = np.random.default_rng(seed)
    seeds = np.pad(rng.random((h, w)) < density, 1)
    grown = np.zeros((h, w), bool)
    for dy in range(3):
        for dx in range(3):
            grown |= seeds[dy:dy + h, dx:dx + w]
    return (grown * rng.integers(1, 3, (h, w))).astype(np.uint8)


def _same_rows(got, want, what=None):
    assert len(got) == 3
    for name, x, y in zip("abn", got, want):
        assert isinstance(x, np.ndarray) and x.dtype == np.int64 and x.shape == y.shape and np.array_equal(x, y), (name, what)


def _check(la, lb, what=None):
    """``ops.patch_overlaps`` of two host planes against the host; neither device plane is written"""
    from deadtrees_amd import ops
    from deadtrees_amd.deployment.overlaps import overlap_pairs_host
    da, db = _dev(la), _dev(lb)
    got = ops.patch_overlaps(da, db)
    want = overlap_pairs_host(la, lb)
    _same_rows(got, want, what)
    assert np.array_equal(da.cpu().numpy(), la) and np.array_equal(db.cpu().numpy(), lb)
    return got


# ---------------------------------------------------------------------------------------------- 1. the kernels alone
def test_one_pixel():
    one = np.ones((1, 1), np.int32)
    got = _check(one, one)
    assert [v.tolist() for v in got] == [[0], [0], [1]]
    assert all(len(v) == 0 for v in _check(one, np.zeros((1, 1), np.int32)))


@pytest.mark.parametrize("transpose", [False, True])
def test_a_row_and_a_column_across_two_chunk_borders(transpose):
    from deadtrees_amd import ops
    C = ops.OVERLAP_CHUNK
    assert C == 1024
    n = 2 * C + 1
    a = np.zeros((1, n), np.uint8)
    b = np.zeros((1, n), np.uint8)
    a[0, 5:C + 3] = 1               # across the first border
    a[0, C + 3:2 * C] = 2           # touches it, another class: a key change inside a chunk
    a[0, 2 * C] = 1                 # the last pixel alone in its chunk
    b[0, C - 1:] = 1                # starts one pixel before the first border, runs through the second
    b[0, 0:3] = 2
    if transpose:
        a, b = a.T, b.T
    got = _check(_labels(a), _labels(b), transpose)
    assert got[2].tolist() == [4, C - 3, 1]
    # a border between two runs of the same pair, and between two different pairs
    for cut in (C, 2 * C):
        a = np.ones((1, n), np.uint8)
        b = np.ones((1, n), np.uint8)
        b[0, cut - 1] = 0
        a2 = a.copy()
        a2[0, cut:] = 2
        for x in (a, a2):
            la, lb = _labels(x), _labels(b)
            _check(la.T if transpose else la, lb.T if transpose else lb, (cut, transpose))


def test_an_odd_pixel_count_reads_its_tail():
    for seed in (0, 1):
        a, b = _blobs(37, 53, seed, 0.1), _blobs(37, 53, seed + 10, 0.1)
        a[-1, -3:] = 1                                  # the last three pixels: behind the last full 16-byte load
        b[-1, -2:] = 2
        got = _check(_labels(a), _labels(b, 4), seed)
        assert len(got[0]) > 5 and (37 * 53) % 4 == 1


def test_a_run_that_wraps_a_row_end_and_a_chunk_border():
    from deadtrees_amd import ops
    w = ops.OVERLAP_CHUNK + 1
    a = np.zeros((3, w), np.uint8)
    a[0, -2:] = 1                   # the end of row 0 (across the chunk border) ...
    a[1, :3] = 2                    # ... and the start of row 1 are two patches: the key changes at the row end
    b = np.ones((3, w), np.uint8)
    la, lb = _labels(a), _labels(b)
    got = _check(la, lb)
    assert [v.tolist() for v in got] == [[w - 2, w], [0, 0], [2, 3]]
    # one patch on both sides of every row end: the run wraps, the pair stays one row
    ring = np.zeros((3, w), np.uint8)
    ring[:, 0] = ring[:, -1] = ring[0] = 1
    got = _check(_labels(ring), lb)
    assert [v.tolist() for v in got] == [[0], [0], [w + 4]]


def test_every_pixel_a_run():
    yy, xx = np.mgrid[0:64, 0:96]
    board = ((yy + xx) % 2).astype(np.uint8)
    la = _labels(board, 4)
    lb = _labels(np.ones((64, 96), np.uint8))
    got = _check(la, lb)
    assert len(got[0]) == 3072 and (got[2] == 1).all() and (got[1] == 0).all()
    _check(lb, la)                                      # the other way round: b varies, a is constant


def test_roots_above_two_to_the_sixteen():
    a = np.zeros((300, 300), np.uint8)
    b = np.zeros((300, 300), np.uint8)
    a[1, 1:4] = 1
    a[297:299, 10:20] = 1
    a[297:300, 200:203] = 2
    b[1, 2:6] = 2
    b[296:300, 15:18] = 1
    b[299, 190:260] = 1
    b[290:298, 201] = 2
    la, lb = _labels(a), _labels(b)
    got = _check(la, lb)
    assert got[0].max() > 2 ** 16 and got[1].max() > 2 ** 16
    assert got[2].tolist() == [2, 6, 1, 3]


@pytest.mark.parametrize("seed", [3, 4, 5])
def test_random_blobs_connectivity_4_against_8(seed):
    a, b = _blobs(96, 160, seed), np.roll(_blobs(96, 160, seed + 100), (2, 3), (0, 1))
    got = _check(_labels(a, 4), _labels(b, 8), seed)
    assert len(got[0]) > 20
    _check(_labels(a, 4), _labels(a, 8), seed)          # the same map: every 4-patch lies in one 8-patch


def test_planes_without_overlap():
    zero = np.zeros((37, 53), np.int32)
    la = _labels(_blobs(37, 53, 7))
    assert all(len(v) == 0 for v in _check(zero, zero))
    assert all(len(v) == 0 for v in _check(la, zero))
    assert all(len(v) == 0 for v in _check(zero, la))
    lb = la.copy()
    lb[la != 0] = 0
    lb[la == 0] = 1                                      # complementary patches: runs everywhere, no pair
    assert all(len(v) == 0 for v in _check(la, lb))


def test_views_and_repetition():
    from deadtrees_amd import ops
    from deadtrees_amd.deployment.overlaps import overlap_pairs_host
    a, b = _blobs(96, 160, 11), _blobs(96, 160, 12)
    la, lb = _labels(a), _labels(b, 4)
    da, db = _dev(la), _dev(lb)
    crop = (slice(5, 90), slice(3, 150, 2))                                      # non-contiguous: made contiguous
    assert not da[crop].is_contiguous()
    _same_rows(ops.patch_overlaps(da[crop], db[crop]),
               overlap_pairs_host(np.ascontiguousarray(la[crop]), np.ascontiguousarray(lb[crop])))
    rows = (slice(1, 95), slice(None))                                           # contiguous at a storage offset
    assert da[rows].is_contiguous() and da[rows].storage_offset() == 160
    _same_rows(ops.patch_overlaps(da[rows], db[rows]),
               overlap_pairs_host(np.ascontiguousarray(la[rows]), np.ascontiguousarray(lb[rows])))
    odd = torch.zeros(37 * 53 + 1, dtype=torch.int32, device=DEV)               # a plane 4 bytes off a 16-byte boundary
    ha = _labels(_blobs(37, 53, 13))
    odd[1:] = _dev(ha).view(-1)
    view = odd[1:].view(37, 53)
    assert view.data_ptr() % 16 == 4
    _same_rows(ops.patch_overlaps(view, view), overlap_pairs_host(ha, ha))
    first, second = ops.patch_overlaps(da, db), ops.patch_overlaps(da, db)
    _same_rows(first, second)
    _same_rows(first, overlap_pairs_host(la, lb))
    assert np.array_equal(da.cpu().numpy(), la) and np.array_equal(db.cpu().numpy(), lb)


def test_argument_errors_are_raised_on_the_host():
    from deadtrees_amd import _lib, ops
    la = _dev(_labels(_blobs(37, 53, 7)))
    for bad in ((la.long(), la), (la, la.long()), (la[:, :-1], la), (la.view(-1), la.view(-1)), (la.cpu(), la),
                (la, la.cpu()), (la[:0], la[:0])):
        with pytest.raises(RuntimeError):
            ops.patch_overlaps(*bad)
    # the entry points refuse a raster beyond int32 labels, and a plane off a 16-byte boundary, before any launch
    lib = _lib.load()
    counts = torch.zeros((4, 2), dtype=torch.int32, device=DEV)
    assert lib.dt_overlap_count(la.data_ptr(), la.data_ptr(), 70000, 70000, counts.data_ptr(), _lib.stream()) != 0
    assert b"2^31-2" in lib.dt_last_error()
    assert lib.dt_overlap_count(la.data_ptr(), la.data_ptr(), 0, 5, counts.data_ptr(), _lib.stream()) != 0
    assert lib.dt_overlap_count(la.data_ptr() + 4, la.data_ptr(), 4, 4, counts.data_ptr(), _lib.stream()) != 0
    assert b"16-byte" in lib.dt_last_error()
    assert not counts.any()
    assert ops.OVERLAP_CHUNK == 1024


# ---------------------------------------------------------------------------------------------- 2. maps in, table out
def _square(y, x, r):
    return [(x - r, y - r), (x + r, y - r), (x + r, y + r), (x - r, y + r)]


@pytest.mark.parametrize("min_a,min_b", [(0, 0), (6, 0), (0, 12), (6, 12)])
def test_patch_overlaps_on_the_device_against_the_host(min_a, min_b):
    from deadtrees_amd.data.polygons import PolygonSet
    from deadtrees_amd.deployment.overlaps import patch_overlaps
    from deadtrees_amd.deployment.patches import PatchConfig
    a, b = _blobs(97, 131, 21, 0.03), np.roll(_blobs(97, 131, 21, 0.03), (1, 2), (0, 1))
    b[40:60, 40:70] = 2
    ca, cb = PatchConfig(4, min_a), PatchConfig(8, min_b)
    want = patch_overlaps(a, b, K, ca, cb)
    assert len(want) > 10 and (min_a == 0 or want.table_a.area.min() >= min_a)
    keep_a, keep_b = a.copy(), b.copy()
    got = patch_overlaps(a, b, K, ca, cb, device=DEV)
    assert got == want and got.table_a == want.table_a and got.table_b == want.table_b
    da, db = _dev(a), _dev(b)
    assert patch_overlaps(da, db, K, ca, cb) == want                              # device tensors choose the device route
    assert np.array_equal(da.cpu().numpy(), keep_a) and np.array_equal(db.cpu().numpy(), keep_b)
    assert np.array_equal(a, keep_a) and np.array_equal(b, keep_b)
    rng = np.random.default_rng(5)
    polys = PolygonSet.from_polygons([(1 + k % 2, _square(rng.uniform(5, 90), rng.uniform(5, 125), rng.uniform(1.5, 6)))
                                      for k in range(25)])
    want = patch_overlaps(polys, b, K, ca, cb)
    assert len(want) > 3
    assert patch_overlaps(polys, b, K, ca, cb, device=DEV) == want
    assert patch_overlaps(polys, db, K, ca, cb) == want
    assert patch_overlaps(polys, polys, K, ca, cb, device=DEV, shape=(97, 131)) == \
        patch_overlaps(polys, polys, K, ca, cb, shape=(97, 131))


# ---------------------------------------------------------------------------------------------- 3. end to end
PATHS = {
    "blocks": dict(overlap=0),
    "crop": dict(overlap=16, blend="crop"),
    "average": dict(overlap=16, blend="average"),
    "tta": dict(tta="flips"),
    "hard vote": dict(overlap=16, blend="crop"),
}
SMALL = (132, 77, 43)      # h * w is a multiple of 4, which the ensemble vote asks for


def _host_overlaps(other, final_map, config, other_config):
    from deadtrees_amd.deployment.overlaps import patch_overlaps
    return patch_overlaps(other, final_map, 2, other_config, config)


@pytest.mark.parametrize("case", list(PATHS))
def test_infer_tile_against_on_every_path(inf, ensemble, case):
    from deadtrees_amd.deployment.patches import PatchConfig
    from deadtrees_amd.deployment.tiler import infer_tile
    raster = tp._raster(*SMALL)
    model = ensemble if case == "hard vote" else inf
    assert case != "hard vote" or ensemble.vote == "hard"
    kw = dict(subtile=tp.D, batch_size=16, device=DEV, stats=True, **PATHS[case])
    other = np.roll(infer_tile(inf, raster, subtile=tp.D, batch_size=16, device=DEV), (2, 3), (0, 1))
    keep = other.copy()
    for config, other_config in ((PatchConfig(8, 0), None), (PatchConfig(4, 4), PatchConfig(8, 3))):
        without = infer_tile(model, raster, patches=config, outlines=True, **kw)
        got = infer_tile(model, raster, patches=config, outlines=True, against=other, against_patches=other_config, **kw)
        assert without[-1].overlaps is None and len(got) == len(without)
        assert got[0].dtype == np.uint8 and np.array_equal(got[0], without[0])
        assert got[-1].patches == without[-1].patches and np.array_equal(got[-1].counts, without[-1].counts)
        for name in ("xy", "ring_offsets", "ring_polygon", "values"):
            assert np.array_equal(getattr(got[-1].outlines, name), getattr(without[-1].outlines, name)), name
        want = _host_overlaps(other, got[0], config, other_config or PatchConfig(config.connectivity))
        assert got[-1].overlaps == want, (case, config)
        assert got[-1].overlaps.table_b == got[-1].patches
        assert np.array_equal(other, keep)
        assert len(want) > 0 and want.table_a.n > 0 and want.table_b.n > 0       # a table worth comparing


def test_infer_tile_against_polygons_and_infer_rasters_with_a_mapping(inf):
    from deadtrees_amd.data.polygons import PolygonSet, rasterize_host
    from deadtrees_amd.deployment.patches import PatchConfig
    from deadtrees_amd.deployment.tiler import infer_rasters, infer_tile
    queue = [("a", tp._raster(*SMALL)), ("b", tp._raster(64, 200, 47))]
    kw = dict(subtile=tp.D, batch_size=16, device=DEV, overlap=16, blend="crop", stats=True, patches=PatchConfig(8, 3))
    rng = np.random.default_rng(9)
    polys = PolygonSet.from_polygons([(1, _square(rng.uniform(5, 125), rng.uniform(5, 70), rng.uniform(1.5, 8)))
                                      for k in range(30)])
    burnt = rasterize_host(polys, SMALL[0], SMALL[1], all_touched=True)
    from_polys = infer_tile(inf, queue[0][1], against=polys, **kw)
    from_array = infer_tile(inf, queue[0][1], against=burnt, **kw)
    assert from_polys[1] == from_array[1] and len(from_polys[1].overlaps) > 5
    assert from_polys[1].overlaps == _host_overlaps(burnt, from_polys[0], PatchConfig(8, 3), PatchConfig(8))
    previous = {"b": np.roll(infer_tile(inf, queue[1][1], subtile=tp.D, batch_size=16, device=DEV), 2, 1)}
    plain = dict(infer_rasters(inf, queue, **kw))
    got = dict(infer_rasters(inf, queue, against=previous, **kw))
    assert got["a"][1] == plain["a"][1] and got["a"][1].overlaps is None          # a missing key: no map to compare with
    assert np.array_equal(got["b"][0], plain["b"][0]) and got["b"][1].patches == plain["b"][1].patches
    assert got["b"][1].overlaps == _host_overlaps(previous["b"], got["b"][0], PatchConfig(8, 3), PatchConfig(8))
    assert dict(infer_rasters(inf, queue, against=previous.get, **kw))["b"][1] == got["b"][1]
    assert (got["a"][1] + got["b"][1]).overlaps is None
    blank = np.zeros((4, 64, 64), np.uint8)
    assert infer_tile(inf, blank, skip_blank=True, against=np.zeros((64, 64), np.uint8), **kw) is None
    for bad in (dict(against=burnt[:, :-1]), dict(against=burnt.astype(np.int32)), dict(against=burnt + 2),
                dict(against_patches=PatchConfig())):
        with pytest.raises(ValueError):
            infer_tile(inf, queue[0][1], **{**kw, **bad})
    with pytest.raises(ValueError):
        infer_tile(inf, queue[0][1], **{**kw, "patches": None, "against": burnt})
    with pytest.raises(ValueError):
        next(infer_rasters(inf, queue, **{**kw, "patches": None, "against": previous}))
