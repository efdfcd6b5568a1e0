"""Overlap-stitched tiled inference, the part that needs no GPU: the window geometry (``window_grid`` / ``blend_ramp`` /
``window_keep`` in numpy against the library's own count), the C ABI of csrc/stitch.hip and its host-side validation."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from deadtrees_amd.deployment.tiler import blend_ramp, infer_rasters, infer_tile, window_grid, window_keep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(300, 470, 128, 32), (300, 470, 128, 64), (512, 512, 256, 64), (200, 330, 64, 16), (64, 64, 64, 32)]
STITCH_SYMBOLS = ["dt_stitch_window_count", "dt_window_normalize_u8", "dt_stitch_accumulate", "dt_stitch_finalize",
                  "dt_stitch_classes_u8"]


def _sweep():
    """(L, d, o) well beyond the listed shapes: every even overlap up to d/2, lengths around every multiple of the stride"""
    for d in (2, 4, 8, 32, 64, 128, 256):
        for o in range(0, d // 2 + 1, 2):
            s = d - o
            lengths = {1, 2, o, o + 1, d - 1, d, d + 1, 2048}
            for m in (1, 2, 3, 7):
                lengths |= {m * s + o - 1, m * s + o, m * s + o + 1, m * s, m * s + d}
            for L in sorted(v for v in lengths if v > 0):
                yield L, d, o


def test_window_count_covers_the_axis_and_has_no_idle_window():
    for L, d, o in _sweep():
        n, _, s = window_grid(L, L, d, o)
        assert s == d - o and n >= 1
        assert (n - 1) * s + d >= L, (L, d, o, n)                # the last window reaches the end
        if n > 1:
            assert (n - 1) * s + o < L, (L, d, o, n)             # ... and sees pixels its neighbour's overlap does not
    for h, w, d, o in SHAPES:
        ny, nx, s = window_grid(h, w, d, o)
        assert (ny, nx) == (window_grid(h, h, d, o)[0], window_grid(w, w, d, o)[0])
        assert (ny - 1) * s + d >= h and (nx - 1) * s + d >= w


def test_no_overlap_is_the_block_grid():
    for h, w, d in [(300, 470, 128), (512, 512, 256), (64, 64, 64), (1, 1, 32), (2048, 2047, 256), (257, 255, 256)]:
        assert window_grid(h, w, d, 0) == (-(-h // d), -(-w // d), d)
        assert window_grid(h, w, d) == window_grid(h, w, d, 0)
        assert np.array_equal(blend_ramp(d, 0), np.ones(d))
    assert [window_keep(i, 3, 64, 0) for i in range(3)] == [(0, 64), (64, 128), (128, 192)]


def test_at_most_two_windows_cover_a_pixel_per_axis():
    for L, d, o in _sweep():
        n, _, s = window_grid(L, L, d, o)
        cover = np.zeros((n - 1) * s + d, dtype=np.int64)
        for i in range(n):
            cover[i * s:i * s + d] += 1
        assert cover.min() >= 1 and cover.max() <= 2, (L, d, o)


def test_ramp_sums_to_one_across_every_interior_overlap():
    for L, d, o in _sweep():
        n, _, s = window_grid(L, L, d, o)
        r = blend_ramp(d, o)
        assert r.dtype == np.float64 and r.shape == (d,) and r.min() > 0 and r.max() <= 1
        total = np.zeros((n - 1) * s + d)
        for i in range(n):
            total[i * s:i * s + d] += r
        interior = total[o:(n - 1) * s + d - o]       # the outer edges of the first / last window have no partner
        assert np.abs(interior - 1.0).max() <= 1e-12 if interior.size else True, (L, d, o)
        for i in range(1, n):                         # the overlaps themselves
            assert np.abs(total[i * s:i * s + o] - 1.0).max() <= 1e-12 if o else True


def test_crop_regions_cover_every_pixel_exactly_once():
    for L, d, o in _sweep():
        n, _, s = window_grid(L, L, d, o)
        cover = np.zeros((n - 1) * s + d, dtype=np.int64)
        for i in range(n):
            lo, hi = window_keep(i, n, d, o)
            assert i * s <= lo < hi <= i * s + d           # inside the window
            cover[lo:hi] += 1
        assert (cover == 1).all(), (L, d, o)
    for h, w, d, o in SHAPES:                              # in 2-D, on the listed shapes
        ny, nx, s = window_grid(h, w, d, o)
        cover = np.zeros(((ny - 1) * s + d, (nx - 1) * s + d), dtype=np.int64)
        for i, j in itertools.product(range(ny), range(nx)):
            (y0, y1), (x0, x1) = window_keep(i, ny, d, o), window_keep(j, nx, d, o)
            cover[y0:y1, x0:x1] += 1
        assert (cover == 1).all()


def test_geometry_arguments_are_validated():
    for bad in (1, 31, -2):
        with pytest.raises(ValueError):
            window_grid(300, 470, 128, bad)
        with pytest.raises(ValueError):
            blend_ramp(128, bad)
    with pytest.raises(ValueError):
        window_grid(300, 470, 128, 66)                    # > d/2
    with pytest.raises(ValueError):
        blend_ramp(64, 34)
    assert window_grid(300, 470, 128, 64) == (4, 7, 64)   # d/2 itself is allowed


def test_reference_import_surface_reexports_the_helpers():
    import deadtrees.deployment.tiler as shim
    assert shim.window_grid is window_grid and shim.blend_ramp is blend_ramp


def test_library_window_count_is_the_python_one():
    """the kernels' own count (dt_stitch_window_count) against window_grid: one geometry in both languages"""
    from deadtrees_amd import _lib
    lib = _lib.load()
    for L, d, o in _sweep():
        assert lib.dt_stitch_window_count(L, d, o) == window_grid(L, L, d, o)[0], (L, d, o)


def test_stitch_entry_points_are_declared_bound_and_exported():
    """header, binding table and shared library agree on the new names (tests/test_abi.py compares the full lists)"""
    from deadtrees_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "deadtrees_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in STITCH_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(raw, name), name
    from deadtrees_amd import ops
    for name in ("window_normalize_u8", "stitch_accumulate", "stitch_finalize", "stitch_classes"):
        assert callable(getattr(ops, name))


def test_host_side_validation_without_gpu():
    """every stitch entry point rejects a bad geometry on the host, before any launch: no GPU is needed to see the error
    (the pointers are never dereferenced on the host; they only have to be non-null)"""
    from deadtrees_amd import _lib
    lib = _lib.load()
    EINVAL = -22
    p = ctypes.c_void_p(4096)
    mean = (ctypes.c_float * 3)(0.5, 0.5, 0.5)

    def err():
        return lib.dt_last_error()

    assert lib.dt_stitch_window_count(300, 128, 31) == EINVAL and b"even" in err()
    assert lib.dt_stitch_window_count(300, 128, 66) == EINVAL and b"d/2" in err()
    assert lib.dt_stitch_window_count(0, 128, 32) == EINVAL
    # gather: stride = d - o
    assert lib.dt_window_normalize_u8(p, p, 4, 300, 470, 128, 97, 5, 0, 1, 3, mean, mean, None, 0, None) == EINVAL and b"even" in err()
    assert lib.dt_window_normalize_u8(p, p, 4, 300, 470, 128, 62, 7, 0, 1, 3, mean, mean, None, 0, None) == EINVAL and b"d/2" in err()
    assert lib.dt_window_normalize_u8(p, p, 4, 300, 470, 128, 129, 4, 0, 1, 3, mean, mean, None, 0, None) == EINVAL
    assert lib.dt_window_normalize_u8(p, p, 4, 300, 470, 128, 96, 4, 0, 1, 3, mean, mean, None, 0, None) == EINVAL and b"nwx" in err()
    ny, nx, s = window_grid(300, 470, 128, 32)
    assert lib.dt_window_normalize_u8(p, p, 4, 300, 470, 128, s, nx, 1, ny * nx, 3, mean, mean, None, 0, None) == EINVAL
    assert b"outside the grid" in err()
    assert lib.dt_window_normalize_u8(None, p, 4, 300, 470, 128, s, nx, 0, 1, 3, mean, mean, None, 0, None) == EINVAL
    assert lib.dt_split_normalize_u8(p, p, 4, 300, 470, 128, 4, 0, 13, 3, mean, mean, None) == EINVAL   # 3 x 4 blocks
    # accumulate / finalize / crop scatter
    assert lib.dt_stitch_accumulate(p, p, 2, 300, 470, 128, 33, 0, 1, None, 0, 0, None) == EINVAL and b"even" in err()
    assert lib.dt_stitch_accumulate(p, p, 2, 300, 470, 128, 66, 0, 1, None, 0, 0, None) == EINVAL and b"d/2" in err()
    assert lib.dt_stitch_accumulate(p, p, 5, 300, 470, 128, 32, 0, 1, None, 0, 0, None) == EINVAL and b"K" in err()
    assert lib.dt_stitch_accumulate(p, p, 2, 300, 470, 128, 32, ny * nx - 1, 2, None, 0, 0, None) == EINVAL
    assert b"outside the grid" in err()
    assert lib.dt_stitch_accumulate(p, None, 2, 300, 470, 128, 32, 0, 1, None, 0, 0, None) == EINVAL
    assert lib.dt_stitch_finalize(p, p, None, 5, 300, 470, None) == EINVAL and b"K" in err()
    assert lib.dt_stitch_finalize(p, None, None, 2, 300, 470, None) == EINVAL
    assert lib.dt_stitch_classes_u8(p, p, 300, 470, 128, 33, 0, 1, None) == EINVAL and b"even" in err()
    assert lib.dt_stitch_classes_u8(p, p, 300, 470, 128, 66, 0, 1, None) == EINVAL and b"d/2" in err()
    assert lib.dt_stitch_classes_u8(p, p, 300, 470, 128, 32, 0, ny * nx + 1, None) == EINVAL
    assert b"outside the grid" in err()


def test_host_side_validation_of_the_merged_entries_without_gpu():
    """the gather and the accumulate take the views themselves: NULL views are the identity view and need n_views == 0, a
    view list needs 1..8 pairs, the weight mode is one of the two constants — all refused by the argument checks, before
    any launch"""
    from deadtrees_amd import _lib
    lib = _lib.load()
    EINVAL = -22
    p = ctypes.c_void_p(4096)
    mean = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    ny, nx, s = window_grid(300, 470, 128, 32)
    ident = (ctypes.c_int * 18)()                      # up to nine identity views

    def gather(views, n_views):
        return lib.dt_window_normalize_u8(p, p, 4, 300, 470, 128, s, nx, 0, 1, 3, mean, mean, views, n_views, None)

    def accumulate(views, n_views, mode=0):
        return lib.dt_stitch_accumulate(p, p, 2, 300, 470, 128, 32, 0, 1, views, n_views, mode, None)

    for call in (gather, accumulate):
        for n_views in (1, 8, -1):
            assert call(None, n_views) == EINVAL and b"n_views == 0" in lib.dt_last_error(), n_views
        for n_views in (0, 9, -1):
            assert call(ident, n_views) == EINVAL and b"1..8" in lib.dt_last_error(), n_views
    for views, n_views in ((None, 0), (ident, 1)):
        for mode in (2, -1):
            assert accumulate(views, n_views, mode) == EINVAL and b"weight_mode" in lib.dt_last_error(), (n_views, mode)


def test_infer_tile_rejects_bad_overlap_requests_before_touching_a_device():
    class _Inf:
        def run_windows(self, *a, **k):          # never reached
            raise AssertionError("validation must come first")

    class _Blocks:
        def run_blocks(self, *a, **k):
            raise AssertionError("validation must come first")

    arr = np.zeros((4, 200, 330), np.uint8)
    with pytest.raises(ValueError, match="even"):
        infer_tile(_Inf(), arr, subtile=128, overlap=31)
    with pytest.raises(ValueError, match="d/2"):
        infer_tile(_Inf(), arr, subtile=128, overlap=66)
    with pytest.raises(ValueError, match="single-rank"):
        infer_tile(_Inf(), arr, subtile=128, overlap=32, world=2, rank=1)
    with pytest.raises(ValueError, match="blend"):
        infer_tile(_Inf(), arr, subtile=128, overlap=32, blend="max")
    with pytest.raises(ValueError, match="return_probs"):
        infer_tile(_Inf(), arr, subtile=128, overlap=32, blend="crop", return_probs=True)
    with pytest.raises(ValueError, match="run_windows"):
        infer_tile(_Blocks(), arr, subtile=128, overlap=32)
    with pytest.raises(ValueError, match="uint8"):
        infer_tile(_Inf(), arr.astype(np.float32), subtile=128, overlap=32)
    with pytest.raises(ValueError, match="even"):
        list(infer_rasters(_Inf(), [arr], subtile=128, overlap=3))
