"""Dead-tree patches on the device: ``csrc/patches.hip`` through ``ops.label_patches`` / ``patch_areas`` / ``sieve_patches`` /
``patch_table`` against the host functions of ``deployment/patches.py`` (themselves pinned to a flood fill in
tests/test_patches_host.py), and ``infer_tile`` / ``infer_rasters`` with ``patches=`` on every device path.  Integers only:
every comparison is exact.

Shapes: a single pixel, single rows and columns, two odd rasters, and the tile ``(th, tw) = ops.PATCH_TILE`` of the local
launch from just below to just above it, 2 x 2 tiles and a bit (the first map with a tile corner inside), and three tile
rows with a ragged last one.  No map exceeds 300 x 470."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
CONNECTIVITIES = (4, 8)


def _shapes():
    from deadtrees_amd import ops
    th, tw = ops.PATCH_TILE
    shapes = [(1, 1), (1, 70), (70, 1), (97, 131), (257, 300),
              (th - 1, tw - 1), (th, tw), (th + 1, tw + 1), (2 * th + 1, 2 * tw + 1), (3 * th - 1, tw + 1)]
    assert all(h <= 300 and w <= 470 for h, w in shapes)
    return shapes


def _spiral(h, w):
    """a square spiral, one pixel wide with one pixel between its laps: walk ahead while the cell two steps on is free"""
    a = np.zeros((h, w), np.uint8)
    y = x = 0
    dy, dx = 0, 1
    a[0, 0] = 1

    def free(yy, xx):
        return not (0 <= yy < h and 0 <= xx < w) or a[yy, xx] == 0

    def ahead(dy, dx):
        return (0 <= y + dy < h and 0 <= x + dx < w and a[y + dy, x + dx] == 0 and free(y + 2 * dy, x + 2 * dx))

    while True:
        if not ahead(dy, dx):
            dy, dx = dx, -dy                                                     # turn right
            if not ahead(dy, dx):
                return a
        y, x = y + dy, x + dx
        a[y, x] = 1


def _serpentine(h, w):
    """rows 0, 2, 4, ... full; the odd rows hold the one pixel that links them, at alternating ends"""
    a = np.zeros((h, w), np.uint8)
    a[0::2] = 1
    for y in range(1, h, 2):
        a[y, w - 1 if (y // 2) % 2 == 0 else 0] = 1
    return a


PATTERNS = ("background", "all one", "checkerboard 0/1", "checkerboard 1/2", "serpentine", "serpentine transposed", "comb",
            "spiral", "diagonal", "anti-diagonal", "random 0.59", "random 0.03")


@functools.lru_cache(maxsize=None)
def _map(pattern, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    if pattern == "background":
        a = np.zeros((h, w))
    elif pattern == "all one":
        a = np.ones((h, w))
    elif pattern == "checkerboard 0/1":
        a = (yy + xx) & 1
    elif pattern == "checkerboard 1/2":
        a = 1 + ((yy + xx) & 1)
    elif pattern == "serpentine":
        a = _serpentine(h, w)
    elif pattern == "serpentine transposed":
        a = _serpentine(w, h).T
    elif pattern == "comb":                                                      # the teeth meet only in the last row
        a = (xx % 2 == 0) | (yy == h - 1)
    elif pattern == "spiral":
        a = _spiral(h, w)
    elif pattern == "diagonal":
        a = yy == xx
    elif pattern == "anti-diagonal":
        a = xx == w - 1 - yy
    else:
        fill = float(pattern.split()[1])
        rng = np.random.default_rng(1000 * h + w + int(100 * fill))
        a = np.where(rng.random((h, w)) < fill, rng.integers(1, 3, (h, w)), 0)
    a = np.ascontiguousarray(a, dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _host(pattern, h, w, connectivity, K=3):
    """(labels, table) of the host contract, computed once"""
    from deadtrees_amd.deployment.patches import label_patches_host, measure_patches_host
    c = _map(pattern, h, w)
    labels = label_patches_host(c, K, connectivity)
    labels.setflags(write=False)
    return labels, measure_patches_host(labels, c)


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)                  # a copy: the cached maps are read-only


def _area_plane_host(labels):
    return np.bincount(labels.ravel(), minlength=labels.size + 1)[1:] * (labels.ravel() == np.arange(1, labels.size + 1))


# ---------------------------------------------------------------------------------------------- 1. labels, areas, table
@pytest.mark.parametrize("pattern", PATTERNS)
def test_labels_areas_and_table_against_the_host(pattern):
    from deadtrees_amd import ops
    for h, w in _shapes():
        for conn in CONNECTIVITIES:
            c = _map(pattern, h, w)
            want_labels, want_table = _host(pattern, h, w, conn)
            dc = _dev(c)
            labels, err = ops.label_patches(dc, 3, conn)
            assert labels.dtype == torch.int32 and tuple(labels.shape) == (h, w)
            assert err.dtype == torch.int32 and tuple(err.shape) == (1,) and int(err) == 0
            assert np.array_equal(labels.cpu().numpy(), want_labels), (h, w, conn)
            area = ops.patch_areas(labels)
            assert area.dtype == torch.int32 and tuple(area.shape) == (h * w,)
            assert np.array_equal(area.cpu().numpy(), _area_plane_host(want_labels)), (h, w, conn)
            assert ops.patch_table(labels, dc, area) == want_table, (h, w, conn)
            assert ops.patch_table(labels, dc) == want_table, (h, w, conn)      # takes the areas itself
            assert np.array_equal(dc.cpu().numpy(), c)                           # nothing wrote to the map
            t = want_table
            if pattern == "background":
                assert t.n == 0 and not labels.any()
            elif pattern in ("all one", "serpentine", "serpentine transposed", "comb", "spiral"):
                assert t.n == 1 and t.root[0] == 0                               # one patch whose first pixel is pixel 0
                if pattern == "all one":
                    assert t.area[0] == h * w and t.bbox[0].tolist() == [0, 0, h - 1, w - 1]
            elif pattern == "checkerboard 0/1":
                ones = (h * w) // 2
                assert t.n == (ones if conn == 4 or min(h, w) == 1 else min(ones, 1))
            elif pattern == "checkerboard 1/2":
                assert t.n == (h * w if conn == 4 or min(h, w) == 1 else min(h * w, 2))
            elif pattern in ("diagonal", "anti-diagonal"):
                assert t.n == (min(h, w) if conn == 4 else 1)


def test_a_class_out_of_range_sets_the_flag_and_is_background():
    from deadtrees_amd import ops
    from deadtrees_amd.deployment.patches import label_patches_host, measure_patches_host
    th, tw = ops.PATCH_TILE
    h, w = 2 * th + 1, 2 * tw + 1
    c = _map("random 0.59", h, w).copy()
    assert (c == 2).any()
    for conn in CONNECTIVITIES:
        labels, err = ops.label_patches(_dev(c), 2, conn)
        assert int(err) == 1
        cleaned = np.where(c == 2, 0, c).astype(np.uint8)
        want = label_patches_host(cleaned, 2, conn)
        got = labels.cpu().numpy()
        assert not got[c == 2].any() and np.array_equal(got, want)
        assert ops.patch_table(labels, _dev(cleaned)) == measure_patches_host(want, cleaned)
        again, err2 = ops.label_patches(_dev(cleaned), 2, conn, err=err)          # the flag is ORed into: it stays
        assert err2 is err and int(err) == 1 and np.array_equal(again.cpu().numpy(), want)


def test_views_with_a_storage_offset_and_non_contiguous_slices():
    from deadtrees_amd import ops
    from deadtrees_amd.deployment.patches import label_patches_host, measure_patches_host
    big = _map("random 0.59", 257, 300)
    dbig = _dev(big)
    crop = (slice(7, 251), slice(3, 290, 2))                                     # non-contiguous: made contiguous
    sub = np.ascontiguousarray(big[crop])
    labels, err = ops.label_patches(dbig[crop], 3)
    assert not dbig[crop].is_contiguous() and int(err) == 0
    want = label_patches_host(sub, 3)
    assert np.array_equal(labels.cpu().numpy(), want)
    assert ops.patch_table(labels, dbig[crop]) == measure_patches_host(want, sub)
    # member m of a stacked [M, h, w] tensor with odd h * w: a contiguous view at an odd byte offset
    stack = np.stack([_map(p, 37, 53) for p in ("random 0.59", "random 0.03", "spiral")])
    ds = _dev(stack)
    for m in range(3):
        assert ds[m].is_contiguous() and ds[m].data_ptr() % 2 == m % 2
        labels, err = ops.label_patches(ds[m], 3, 4)
        want = label_patches_host(stack[m], 3, 4)
        assert np.array_equal(labels.cpu().numpy(), want) and int(err) == 0, m
        assert ops.patch_table(labels, ds[m]) == measure_patches_host(want, stack[m]), m
    rows = dbig[40:140]                                                          # a contiguous crop of rows, offset 40 * 300
    assert rows.is_contiguous() and rows.storage_offset() == 40 * 300
    assert np.array_equal(ops.label_patches(rows, 3)[0].cpu().numpy(), label_patches_host(np.ascontiguousarray(big[40:140]), 3))


def test_the_same_call_twice_gives_the_same_labels_and_table():
    from deadtrees_amd import ops
    dc = _dev(_map("random 0.59", 257, 300))
    first, _ = ops.label_patches(dc, 3)
    second, _ = ops.label_patches(dc, 3)
    assert torch.equal(first, second)
    assert ops.patch_table(first, dc) == ops.patch_table(second, dc)


def test_argument_errors_are_raised_on_the_host():
    from deadtrees_amd import ops
    dc = _dev(_map("random 0.03", 97, 131))
    labels, _ = ops.label_patches(dc, 3)
    area = ops.patch_areas(labels)
    for K, conn in ((1, 8), (9, 8), (3, 6), (3, 0)):
        with pytest.raises(RuntimeError):
            ops.label_patches(dc, K, conn)
    with pytest.raises(RuntimeError):
        ops.label_patches(dc.int(), 3)
    with pytest.raises(RuntimeError):
        ops.label_patches(dc.view(-1), 3)
    with pytest.raises(RuntimeError):
        ops.label_patches(dc.cpu(), 3)
    with pytest.raises(RuntimeError):
        ops.patch_areas(labels.long())
    with pytest.raises(RuntimeError):
        ops.sieve_patches(dc, labels[:, :-1], area, 2)
    with pytest.raises(RuntimeError):
        ops.sieve_patches(dc, labels, area[:-1], 2)
    with pytest.raises(RuntimeError):
        ops.sieve_patches(dc, labels, area, -1)
    with pytest.raises(RuntimeError):
        ops.sieve_patches(dc.t(), labels.t(), area, 2)                          # in place needs contiguous tensors
    with pytest.raises(RuntimeError):
        ops.patch_table(labels, dc.int())
    with pytest.raises(RuntimeError):
        ops.patch_table(labels, dc, area.long())
    assert ops.patch_table(labels, dc, area) == _host("random 0.03", 97, 131, 8)[1]   # and nothing was left behind


# ---------------------------------------------------------------------------------------------- 2. the sieve
@pytest.mark.parametrize("min_pixels", [1, 2, 5, "h*w"])
def test_sieve_against_the_host(min_pixels):
    from deadtrees_amd import ops
    from deadtrees_amd.deployment.patches import measure_patches_host, sieve_host
    from deadtrees_amd.deployment.stats import zonal_counts_host
    for pattern in ("random 0.59", "random 0.03"):
        for h, w in _shapes():
            for conn in CONNECTIVITIES:
                m = h * w if min_pixels == "h*w" else min_pixels
                c = _map(pattern, h, w)
                host_labels, _ = _host(pattern, h, w, conn)
                want_c, want_l = sieve_host(c, host_labels, m)
                dc = _dev(c)
                labels, _ = ops.label_patches(dc, 3, conn)
                area = ops.patch_areas(labels)
                ops.sieve_patches(dc, labels, area, m)
                assert np.array_equal(dc.cpu().numpy(), want_c), (pattern, h, w, conn)
                assert np.array_equal(labels.cpu().numpy(), want_l), (pattern, h, w, conn)
                assert np.array_equal(area.cpu().numpy(), _area_plane_host(want_l)), (pattern, h, w, conn)
                table = ops.patch_table(labels, dc, area)
                assert table == measure_patches_host(want_l, want_c), (pattern, h, w, conn)
                assert table.n == 0 or int(table.area.min()) >= m
                counts, err = ops.zonal_counts(dc, None, 3, 1)
                assert np.array_equal(counts.cpu().numpy(), zonal_counts_host(want_c, None, 3, 1)) and int(err) == 0
                if m <= 1:
                    assert np.array_equal(want_c, c)


# ---------------------------------------------------------------------------------------------- 3. end to end
H, W, D = 300, 470, 64


@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    from deadtrees_amd.network.segmodel import SemSegment
    from deadtrees_amd.utils.config import default_network, default_training
    from oracle.unet_ref import make_oracle
    files = []
    for seed in (1, 2, 3):
        model = SemSegment(default_network(), default_training())
        model.model.load_state_dict(make_oracle(3, 2, seed=seed).state_dict())
        files.append(tmp_path_factory.mktemp(f"ckpt{seed}") / "bestmodel.ckpt")
        model.save_checkpoint(files[-1])
    return files


@pytest.fixture(scope="module")
def ensemble(ckpts):
    from deadtrees_amd.deployment.inference import PyTorchEnsembleInference
    return PyTorchEnsembleInference(*ckpts)


@pytest.fixture(scope="module")
def inf(ensemble):
    """the member whose map of the random raster is speckled: 8 - 18 % class 1 in about 2000 patches, most of them below
    four pixels (the first member calls nearly every pixel class 1: one patch)"""
    return ensemble.members[2]


def _raster(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (4, h, w), dtype=np.uint8)


E2E = {
    "blocks": dict(overlap=0),
    "crop": dict(overlap=16, blend="crop"),
    "average": dict(overlap=16, blend="average"),
    "average+probs": dict(overlap=16, blend="average", return_probs=True),
    "tta": dict(tta="flips"),
    "soft vote": dict(overlap=16, blend="average"),
    "host": dict(overlap=0, on_device=False),
}


@pytest.mark.parametrize("case", list(E2E))
def test_infer_tile_patches_on_every_path(inf, ensemble, case):
    from deadtrees_amd.deployment.patches import PatchConfig, label_patches_host, measure_patches_host, sieve_host
    from deadtrees_amd.deployment.stats import zonal_counts_host
    from deadtrees_amd.deployment.tiler import infer_tile
    raster = _raster(H, W, 31)
    model = ensemble if "vote" in case else inf
    kw = dict(subtile=D, batch_size=16, device=DEV, **E2E[case])
    if case == "soft vote":
        ensemble.vote = "soft"
    try:
        base = infer_tile(model, raster, **kw)
        plain = infer_tile(model, raster, stats=True, **kw)
        with_table = infer_tile(model, raster, stats=True, patches=True, **kw)
        four = infer_tile(model, raster, stats=True, patches=PatchConfig(connectivity=4), **kw)
        sieved = infer_tile(model, raster, stats=True, patches=PatchConfig(min_pixels=4), **kw)
    finally:
        ensemble.vote = "hard"
    if case == "average+probs":
        for got in (plain, with_table, sieved):
            assert len(got) == 3 and np.array_equal(got[1], base[1])            # the sieve does not touch the probabilities
        base = base[0]
    else:
        assert len(with_table) == 2 and len(sieved) == 2
    assert base.dtype == np.uint8 and base.shape == (H, W)
    assert plain[-1].patches is None
    labels = label_patches_host(base, 2)
    assert np.array_equal(with_table[0], base) and with_table[0].dtype == np.uint8    # bit-identical to the call without
    assert with_table[-1].patches == measure_patches_host(labels, base)
    if model is inf:                                                             # a map worth labelling and sieving
        assert with_table[-1].patches.n > 100 and int(np.count_nonzero(with_table[-1].patches.area < 4)) > 10
        assert sieved[-1].patches.n < with_table[-1].patches.n and not np.array_equal(sieved[0], base)
    assert np.array_equal(with_table[-1].counts, plain[-1].counts)
    assert np.array_equal(four[0], base) and four[-1].patches == measure_patches_host(label_patches_host(base, 2, 4), base)
    want_c, want_l = sieve_host(base, labels, 4)
    assert np.array_equal(sieved[0], want_c)
    assert sieved[-1].patches == measure_patches_host(want_l, want_c)
    assert np.array_equal(sieved[-1].counts, zonal_counts_host(sieved[0], None, 2, 1))
    assert sieved[-1].patches.n == 0 or int(sieved[-1].patches.area.min()) >= 4


def test_infer_rasters_passes_patches_through_and_patches_need_stats(inf):
    from deadtrees_amd.deployment.patches import PatchConfig, label_patches_host, measure_patches_host, sieve_host
    from deadtrees_amd.deployment.tiler import infer_rasters, infer_tile
    queue = [("a", _raster(130, 77, 43)), ("b", _raster(64, 200, 47))]
    kw = dict(subtile=D, batch_size=16, device=DEV, overlap=16, blend="crop")
    base = dict(infer_rasters(inf, queue, **kw))
    got = dict(infer_rasters(inf, queue, stats=True, patches=PatchConfig(8, 3), **kw))
    for key in ("a", "b"):
        want_c, want_l = sieve_host(base[key], label_patches_host(base[key], 2), 3)
        assert np.array_equal(got[key][0], want_c) and got[key][1].patches == measure_patches_host(want_l, want_c)
    assert (got["a"][1] + got["b"][1]).patches is None
    with pytest.raises(ValueError):
        next(infer_rasters(inf, queue, patches=True, **kw))
    with pytest.raises(ValueError):
        infer_tile(inf, queue[0][1], patches=True, **kw)
    with pytest.raises(ValueError):
        infer_tile(inf, queue[0][1], stats=True, patches="yes", **kw)
