"""Test-time augmentation and ensemble voting on the stitched path, the part that needs no GPU: ``tta_views``, a numpy
restatement of the view / inverse-view pixel maps of csrc/views.h against ``np.rot90`` and slicing, the host-side
validation of the two new C entries, and ``infer_tile``'s argument checks."""
import ctypes

import numpy as np
import pytest

from deadtrees_amd.deployment.tiler import infer_rasters, infer_tile, tta_views, window_grid

D4 = tuple((f, k) for f in (0, 1) for k in range(4))
ALL = D4 + tuple((2, k) for k in range(4))          # the eight views and the four flip = 2 aliases


def source_pixel(flip, rot, y, x, n):
    """csrc/views.h aug_source_pixel on an n x n tile: view[y][x] = tile[sy][sx]"""
    ry, rx = y, x
    if rot == 1:
        ry, rx = x, n - 1 - y
    elif rot == 2:
        ry, rx = n - 1 - y, n - 1 - x
    elif rot == 3:
        ry, rx = n - 1 - x, y
    if flip == 1:
        rx = n - 1 - rx
    elif flip == 2:
        ry = n - 1 - ry
    return ry, rx


def inverse_view(flip, rot):
    """what stitch_pack_views(inverse) packs: rot90^k is undone by rot90^(4-k), a view with a flip by itself"""
    return (flip, rot) if flip else (0, (4 - rot) % 4)


def np_view(tile, flip, rot):
    """view = rot90^rot(flip(tile)) over the last two axes"""
    f = tile[..., :, ::-1] if flip == 1 else tile[..., ::-1, :] if flip == 2 else tile
    return np.rot90(f, rot, axes=(-2, -1))


def test_named_sets_and_canonical_form():
    assert tta_views(None) == ((0, 0),)
    assert tta_views("flips") == ((0, 0), (1, 0), (1, 2), (0, 2))        # identity, horizontal, vertical, both
    assert tta_views("d4") == D4 and len(set(tta_views("d4"))) == 8
    assert tta_views([(0, 0)]) == ((0, 0),)
    assert tta_views([(2, 0), (2, 1), (2, 2), (2, 3)]) == ((1, 2), (1, 3), (1, 0), (1, 1))
    assert tta_views(((0, 3), [1, 1])) == ((0, 3), (1, 1))
    assert tta_views(np.array([[0, 1], [2, 3]])) == ((0, 1), (1, 1))
    assert all(isinstance(v, int) for pair in tta_views(np.array([[0, 1], [2, 3]])) for v in pair)


def test_bad_requests_are_value_errors():
    for bad in ([], (), "rot", "D4", [(0, 4)], [(3, 0)], [(-1, 0)], [(0, -1)], [(0,)], [(0, 0, 0)], [0, 1], [(0.5, 0)],
                [(0, 0), (0, 0)], [(1, 0), (2, 2)], [(2, 1), (1, 3)], list(D4) + [(2, 0)]):
        with pytest.raises(ValueError):
            tta_views(bad)


def test_reference_import_surface_reexports_tta_views():
    import deadtrees.deployment.tiler as shim
    assert shim.tta_views is tta_views


@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_view_and_inverse_pixel_maps_agree_with_numpy(n):
    """for all 8 views and the flip = 2 aliases: the gather's pixel map is np.rot90 of the flipped tile; the accumulate's
    lookup (the inverse view's pixel map) finds every tile pixel in the view; view . inverse is the identity"""
    tile = np.arange(n * n).reshape(n, n)
    ys, xs = np.divmod(np.arange(n * n), n)
    for flip, rot in ALL:
        want = np_view(tile, flip, rot)
        sy, sx = zip(*(source_pixel(flip, rot, y, x, n) for y, x in zip(ys, xs)))
        assert np.array_equal(tile[list(sy), list(sx)].reshape(n, n), want), (flip, rot)
        inv = inverse_view(flip, rot)
        vy, vx = zip(*(source_pixel(*inv, y, x, n) for y, x in zip(ys, xs)))
        assert np.array_equal(want[list(vy), list(vx)].reshape(n, n), tile), (flip, rot)
        assert np.array_equal(np_view(want, *inv), tile) and np.array_equal(np_view(np_view(tile, *inv), flip, rot), tile)
        (canon,) = tta_views([(flip, rot)])
        assert np.array_equal(np_view(tile, *canon), want), (flip, rot)       # (2, k) is (1, (k + 2) % 4)
    if n > 1:
        assert len({np_view(tile, f, k).tobytes() for f, k in D4}) == 8        # the canonical eight are distinct


def test_host_side_validation_of_the_views_entries_without_gpu():
    """both entries reject a bad view list / weight mode on the host before any launch, after the rules of their siblings"""
    from deadtrees_amd import _lib
    lib = _lib.load()
    EINVAL = -22
    p = ctypes.c_void_p(4096)
    mean = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    ny, nx, s = window_grid(300, 470, 128, 32)

    def views(*pairs):
        flat = [v for pair in pairs for v in pair]
        return (ctypes.c_int * max(1, len(flat)))(*flat), len(pairs)

    def gather(arr, T, stride=s, nwx=nx, first=0, count=1):
        return lib.dt_window_normalize_u8(p, p, 4, 300, 470, 128, stride, nwx, first, count, 3, mean, mean, arr, T, None)

    def accumulate(arr, T, mode=0, overlap=32, K=2, first=0, count=1):
        return lib.dt_stitch_accumulate(p, p, K, 300, 470, 128, overlap, first, count, arr, T, mode, None)

    for call in (gather, accumulate):
        assert call(*views()) == EINVAL and b"1..8" in lib.dt_last_error()
        assert call(*views(*([(0, 0)] * 9))) == EINVAL and b"1..8" in lib.dt_last_error()
        assert call(*views((0, 0), (3, 0))) == EINVAL and b"flip" in lib.dt_last_error()
        assert call(*views((-1, 0))) == EINVAL and b"flip" in lib.dt_last_error()
        assert call(*views((0, 0), (1, 4))) == EINVAL and b"rot" in lib.dt_last_error()
        assert call(*views((0, -1))) == EINVAL and b"rot" in lib.dt_last_error()
        assert call(None, 1) == EINVAL
    ok = views(*D4)
    assert accumulate(*ok, mode=2) == EINVAL and b"weight_mode" in lib.dt_last_error()
    assert accumulate(*ok, mode=-1) == EINVAL and b"weight_mode" in lib.dt_last_error()
    # the siblings' rules hold for the new entries
    assert gather(*ok, stride=97, nwx=5) == EINVAL and b"even" in lib.dt_last_error()
    assert gather(*ok, stride=62, nwx=7) == EINVAL and b"d/2" in lib.dt_last_error()
    assert gather(*ok, nwx=nx + 1) == EINVAL and b"nwx" in lib.dt_last_error()
    assert gather(*ok, first=1, count=ny * nx) == EINVAL and b"outside the grid" in lib.dt_last_error()
    assert accumulate(*ok, overlap=33) == EINVAL and b"even" in lib.dt_last_error()
    assert accumulate(*ok, overlap=66) == EINVAL and b"d/2" in lib.dt_last_error()
    assert accumulate(*ok, K=5) == EINVAL and b"K" in lib.dt_last_error()
    assert accumulate(*ok, first=ny * nx - 1, count=2) == EINVAL and b"outside the grid" in lib.dt_last_error()


def test_infer_tile_rejects_bad_tta_and_ensemble_requests_before_touching_a_device():
    class _Inf:
        def run_windows(self, *a, **k):          # never reached
            raise AssertionError("validation must come first")

    class _Blocks:
        def run_blocks(self, *a, **k):
            raise AssertionError("validation must come first")

    class _Ensemble:
        vote = "hard"
        members = (_Inf(), _Inf(), _Inf())

    arr = np.zeros((4, 200, 330), np.uint8)
    with pytest.raises(ValueError, match="tta"):
        infer_tile(_Inf(), arr, subtile=128, tta="rot")
    with pytest.raises(ValueError, match="duplicate"):
        infer_tile(_Inf(), arr, subtile=128, overlap=32, tta=[(1, 0), (2, 2)])
    with pytest.raises(ValueError, match="even"):
        infer_tile(_Inf(), arr, subtile=128, overlap=31, tta="d4")
    with pytest.raises(ValueError, match="single-rank"):
        infer_tile(_Inf(), arr, subtile=128, tta="d4", world=2, rank=1)
    with pytest.raises(ValueError, match="return_probs"):
        infer_tile(_Inf(), arr, subtile=128, overlap=32, tta="d4", blend="crop", return_probs=True)
    with pytest.raises(ValueError, match="return_probs"):
        infer_tile(_Ensemble(), arr, subtile=128, overlap=32, blend="average", return_probs=True)
    with pytest.raises(ValueError, match="run_windows"):
        infer_tile(_Blocks(), arr, subtile=128, tta="flips")
    with pytest.raises(ValueError, match="run_windows"):
        infer_tile(_Inf(), arr, subtile=128, tta="flips", on_device=False)
    with pytest.raises(ValueError, match="uint8"):
        infer_tile(_Inf(), arr.astype(np.float32), subtile=128, tta="flips")
    with pytest.raises(ValueError, match="tta"):
        list(infer_rasters(_Inf(), [arr], subtile=128, tta="nope"))
