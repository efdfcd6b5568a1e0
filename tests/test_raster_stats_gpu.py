"""Raster statistics on the device: ``dt_zonal_counts_u8`` (csrc/raster_stats.hip) through ``ops.zonal_counts`` against
``stats.zonal_counts_host`` (itself pinned to ``np.count_nonzero`` in tests/test_raster_stats_host.py), and
``infer_tile`` / ``infer_rasters`` with ``stats=True`` on every device path.  Integers only: every comparison is exact.

Sizes: below, at and above one 16-byte vector (1, 15, 16, 17) and a few of them with and without a tail (63, 64, 65);
4097 = one full workgroup of 256 vectors and a 1-pixel tail; 300 x 470 (the end-to-end raster: 8812 vectors + 8 pixels, 35
workgroups, the last one ragged) and 512 x 512 (64 workgroups).  The grid is capped at 512 workgroups = 131072 vectors:
test_counts_add_up_over_calls_and_a_grid_stride_loop runs 3 MiB + 5 pixels, where half of the lanes take a second vector."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

SIZES = [1, 15, 16, 17, 63, 64, 65, 4097, 300 * 470, 512 * 512]
KZ = [(2, 1), (3, 1), (3, 3), (8, 8)]


@functools.lru_cache(maxsize=None)
def _maps(n, K, Z, kind):
    """(classes, zones) uint8 [n], seeded; "skewed": 97 % class 0, "uniform": all values equally likely"""
    rng = np.random.default_rng(7 * n + 100 * K + 10 * Z + len(kind))
    if kind == "skewed":
        c = np.where(rng.random(n) < 0.97, 0, rng.integers(1, K, n)).astype(np.uint8)
    else:
        c = rng.integers(0, K, n, dtype=np.uint8)
    z = rng.integers(0, Z, n, dtype=np.uint8)
    c.setflags(write=False)
    z.setflags(write=False)
    return c, z


def _host(c, z, K, Z):
    from deadtrees_amd.deployment.stats import zonal_counts_host
    return zonal_counts_host(c, z, K, Z)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("n", SIZES)
def test_kernel_against_the_host_counts(n):
    from deadtrees_amd import ops
    for K, Z in KZ:
        for kind in ("skewed", "uniform"):
            c, z = _maps(n, K, Z, kind)
            counts, err = ops.zonal_counts(_dev(c), _dev(z), K, Z)
            assert counts.dtype == torch.int64 and tuple(counts.shape) == (Z, K)
            assert err.dtype == torch.int32 and tuple(err.shape) == (1,)
            got = counts.cpu().numpy()
            assert np.array_equal(got, _host(c, z, K, Z)), (K, Z, kind)
            assert int(got.sum()) == n and int(err) == 0
            plain, err = ops.zonal_counts(_dev(c), None, K)                        # without zones: every pixel is zone 0
            assert tuple(plain.shape) == (1, K) and np.array_equal(plain.cpu().numpy(), _host(c, None, K, 1)), (K, kind)
            assert int(err) == 0


def test_any_shape_and_non_contiguous_views():
    from deadtrees_amd import ops
    c, z = _maps(300 * 470, 3, 3, "skewed")
    want = _host(c, z, 3, 3)
    dc, dz = _dev(c.reshape(300, 470)), _dev(z.reshape(300, 470))
    assert np.array_equal(ops.zonal_counts(dc, dz, 3, 3)[0].cpu().numpy(), want)
    assert np.array_equal(ops.zonal_counts(dc.view(3, 100, 470), dz.view(3, 100, 470), 3, 3)[0].cpu().numpy(), want)
    crop = (slice(7, 291), slice(3, 460, 2))                                       # non-contiguous: made contiguous
    got = ops.zonal_counts(dc[crop], dz[crop], 3, 3)[0].cpu().numpy()
    assert np.array_equal(got, _host(c.reshape(300, 470)[crop], z.reshape(300, 470)[crop], 3, 3))
    # member m of a stacked [M, h, w] tensor with odd h * w: a contiguous view at an odd byte offset
    stack = np.stack([_maps(37 * 53, 3, 3, kind)[0].reshape(37, 53) for kind in ("skewed", "uniform", "skewed")])
    zone = _maps(37 * 53, 3, 3, "uniform")[1].reshape(37, 53)
    ds, dzone = _dev(stack), _dev(zone)
    for m in range(3):
        assert ds[m].is_contiguous() and ds[m].data_ptr() % 2 == m % 2
        assert np.array_equal(ops.zonal_counts(ds[m], dzone, 3, 3)[0].cpu().numpy(), _host(stack[m], zone, 3, 3)), m


@pytest.mark.parametrize("n", [4097, 300 * 470])
@pytest.mark.parametrize("a", [1, 3, 5, 16])
def test_misaligned_contiguous_views(n, a):
    """``buf[a:a + n]``: the classes start ``a`` bytes behind a 16-byte boundary, the zones at another offset"""
    from deadtrees_amd import ops
    c, z = _maps(n, 3, 3, "skewed")
    for za in ((a + 7) % 16, a + 2, 0, 15):
        cbuf = torch.full((n + 64,), 200, dtype=torch.uint8, device=DEV)           # out-of-range bytes all around
        zbuf = torch.full((n + 64,), 200, dtype=torch.uint8, device=DEV)
        assert cbuf.data_ptr() % 16 == 0 and zbuf.data_ptr() % 16 == 0
        cbuf[a:a + n] = _dev(c)
        zbuf[za:za + n] = _dev(z)
        cv, zv = cbuf[a:a + n], zbuf[za:za + n]
        assert cv.is_contiguous() and cv.data_ptr() % 16 == a % 16 and zv.data_ptr() % 16 == za % 16
        counts, err = ops.zonal_counts(cv, zv, 3, 3)
        assert np.array_equal(counts.cpu().numpy(), _host(c, z, 3, 3)), (a, za)
        assert int(err) == 0, (a, za)                                              # no byte outside the views was counted
        plain, err = ops.zonal_counts(cv, None, 3)
        assert np.array_equal(plain.cpu().numpy(), _host(c, None, 3, 1)) and int(err) == 0, a


def test_counts_add_up_over_calls_and_a_grid_stride_loop():
    from deadtrees_amd import ops
    c1, z1 = _maps(300 * 470, 3, 3, "skewed")
    c2, z2 = _maps(4097, 3, 3, "uniform")
    counts, err = ops.zonal_counts(_dev(c1), _dev(z1), 3, 3)
    back, err_back = ops.zonal_counts(_dev(c2), _dev(z2), 3, 3, counts=counts, err=err)
    assert back is counts and err_back is err
    got = counts.cpu().numpy()
    assert np.array_equal(got, _host(c1, z1, 3, 3) + _host(c2, z2, 3, 3))
    assert int(got.sum()) == 300 * 470 + 4097 and int(err) == 0
    # 3 MiB + 5: 196608 vectors on the capped grid of 512 x 256 lanes, half of the lanes take a second one
    n = 3 * 1024 * 1024 + 5
    c, z = _maps(n, 3, 2, "skewed")
    got = ops.zonal_counts(_dev(c), _dev(z), 3, 2)[0].cpu().numpy()
    assert np.array_equal(got, _host(c, z, 3, 2)) and int(got.sum()) == n


@pytest.mark.parametrize("what,flag", [("class K", 1), ("class 255", 1), ("zone Z", 2), ("both", 3)])
def test_values_out_of_range_set_the_flag_and_enter_no_count(what, flag):
    from deadtrees_amd import ops
    K, Z, h, w = 3, 3, 300, 470
    c, z = (a.copy() for a in _maps(h * w, K, Z, "skewed"))
    where = np.array([0, 1, 17, 4711, 65536, h * w - 2, h * w - 1])                # head, body and tail of the map
    if what in ("class K", "class 255"):
        c[where] = K if what == "class K" else 255
    elif what == "zone Z":
        z[where] = Z
    else:
        c[where[:3]] = K
        z[where[2:]] = Z                                                          # pixel 17 is wrong in both
    counts, err = ops.zonal_counts(_dev(c.reshape(h, w)), _dev(z.reshape(h, w)), K, Z)
    assert int(err) == flag
    keep = np.ones(h * w, bool)
    keep[where] = False
    got = counts.cpu().numpy()
    assert np.array_equal(got, _host(c[keep], z[keep], K, Z))                      # exactly those pixels are missing
    assert int(got.sum()) == h * w - len(where)


def test_argument_errors_are_raised_on_the_host():
    from deadtrees_amd import ops
    c, z = (_dev(a.reshape(37, 53)) for a in _maps(37 * 53, 3, 3, "uniform"))
    for K, Z, zones in ((1, 1, None), (9, 1, None), (3, 9, z), (3, 0, z), (3, 2, None)):
        with pytest.raises(RuntimeError):
            ops.zonal_counts(c, zones, K, Z)
    with pytest.raises(RuntimeError):
        ops.zonal_counts(c, z[:, :-1], 3, 3)                                       # unequal shapes
    with pytest.raises(RuntimeError):
        ops.zonal_counts(c.long(), z, 3, 3)
    with pytest.raises(RuntimeError):
        ops.zonal_counts(c, z.int(), 3, 3)
    with pytest.raises(RuntimeError):
        ops.zonal_counts(c, z, 3, 3, counts=torch.zeros((3, 2), dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError):
        ops.zonal_counts(c, z, 3, 3, counts=torch.zeros((3, 3), dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError):
        ops.zonal_counts(c.cpu(), z.cpu(), 3, 3)
    counts, err = ops.zonal_counts(c, z, 3, 3)                                     # and nothing was left behind
    assert int(counts.sum()) == 37 * 53 and int(err) == 0


# ---------------------------------------------------------------------------------------------- 2. end to end
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
    return ensemble.members[0]


def _raster(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (4, h, w), dtype=np.uint8)


ZONES = np.random.default_rng(99).integers(0, 3, (H, W), dtype=np.uint8)
ZONES.setflags(write=False)

E2E = {
    "blocks": dict(overlap=0),
    "crop": dict(overlap=16, blend="crop"),
    "average": dict(overlap=16, blend="average"),
    "average+probs": dict(overlap=16, blend="average", return_probs=True),
    "tta": dict(tta="flips"),
    "hard vote": dict(overlap=16, blend="crop"),
    "soft vote": dict(overlap=16, blend="average"),
}


@pytest.mark.parametrize("case", list(E2E))
def test_infer_tile_stats_on_every_device_path(inf, ensemble, case):
    from deadtrees_amd.deployment.stats import RasterStats
    from deadtrees_amd.deployment.tiler import infer_tile
    raster = _raster(H, W, 31)
    model = ensemble if "vote" in case else inf
    assert model.classes == 2
    kw = dict(subtile=D, batch_size=16, device=DEV, **E2E[case])
    if case == "soft vote":
        ensemble.vote = "soft"
    try:
        base = infer_tile(model, raster, **kw)
        with_zones = infer_tile(model, raster, stats=True, zones=ZONES, **kw)
        without = infer_tile(model, raster, stats=True, **kw)
    finally:
        ensemble.vote = "hard"
    if case == "average+probs":
        assert len(with_zones) == 3 and len(without) == 3
        assert np.array_equal(with_zones[1], base[1]) and np.array_equal(without[1], base[1])     # probabilities, bit for bit
        base = base[0]
    else:
        assert len(with_zones) == 2 and len(without) == 2
    assert base.dtype == np.uint8 and base.shape == (H, W)
    for got in (with_zones, without):
        assert got[0].dtype == np.uint8 and np.array_equal(got[0], base)           # the map of the call without stats
        assert isinstance(got[-1], RasterStats)
    assert with_zones[-1].counts.shape == (3, 2) and np.array_equal(with_zones[-1].counts, _host(base, ZONES, 2, 3))
    assert without[-1].counts.shape == (1, 2) and np.array_equal(without[-1].counts, _host(base, None, 2, 1))
    assert with_zones[-1].total == H * W


def test_a_previous_map_as_zones_gives_the_transition_matrix(inf, ensemble):
    from deadtrees_amd.deployment.tiler import infer_tile
    kw = dict(subtile=D, batch_size=16, device=DEV, overlap=16, blend="average")
    prev = infer_tile(ensemble.members[1], _raster(H, W, 31), **kw)
    now, stats = infer_tile(inf, _raster(H, W, 31), stats=True, zones=prev, n_zones=2, **kw)
    assert stats.counts.shape == (2, 2)
    for a in range(2):
        for b in range(2):
            assert stats.counts[a, b] == np.count_nonzero((prev == a) & (now == b)), (a, b)
    with pytest.raises(ValueError):
        infer_tile(inf, _raster(H, W, 31), stats=True, zones=ZONES, n_zones=2, **kw)
    with pytest.raises(ValueError):
        infer_tile(inf, _raster(H, W, 31), zones=ZONES, **kw)


def test_infer_rasters_stats_add_up_over_rasters_and_ranks(inf):
    from deadtrees_amd.deployment.tiler import infer_rasters
    blank = _raster(128, 200, 41)
    blank[0] = np.where(blank[0] > 127, 255, 0)
    queue = [("a", _raster(H, W, 31)), ("blank", blank), ("c", _raster(130, 77, 43))]
    zones = {key: np.random.default_rng(len(key) + arr.shape[1]).integers(0, 3, arr.shape[1:], dtype=np.uint8)
             for key, arr in queue}
    kw = dict(subtile=D, batch_size=16, device=DEV, overlap=16, blend="crop", stats=True, zones=zones, n_zones=3)
    got = dict(infer_rasters(inf, queue, **kw))
    assert list(got) == ["a", "blank", "c"] and got["blank"] is None
    total = got["a"][1] + got["c"][1]
    maps = np.concatenate([got["a"][0].ravel(), got["c"][0].ravel()])
    zone = np.concatenate([zones["a"].ravel(), zones["c"].ravel()])
    assert np.array_equal(total.counts, _host(maps, zone, 2, 3)) and total.total == H * W + 130 * 77
    by_rank = [dict(infer_rasters(inf, queue, rank=r, world=2, **kw)) for r in range(2)]
    assert sorted(by_rank[0]) == ["a", "c"] and list(by_rank[1]) == ["blank"] and by_rank[1]["blank"] is None
    parts = [v[1] for d in by_rank for v in d.values() if v is not None]
    assert parts[0] + parts[1] == total
    queue4 = queue + [("d", _raster(64, 64, 47))]                                  # a fourth raster: both ranks hold counts
    zones["d"] = np.zeros((64, 64), np.uint8)
    whole = [v[1] for v in dict(infer_rasters(inf, queue4, **kw)).values() if v is not None]
    ranks = [[v[1] for v in dict(infer_rasters(inf, queue4, rank=r, world=2, **kw)).values() if v is not None]
             for r in range(2)]
    assert len(ranks[0]) == 2 and len(ranks[1]) == 1
    assert sum(ranks[0][1:], ranks[0][0]) + ranks[1][0] == sum(whole[1:], whole[0])
