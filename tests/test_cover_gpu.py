"""Cover grids on the device: ``dt_cover_grid_u8`` (csrc/cover.hip) through ``ops.cover_grid`` against ``cover_grid_host``
(itself pinned to a scalar restatement of the contract in tests/test_cover_host.py), and ``infer_tile`` / ``infer_rasters``
with ``grid=`` on every device path.  Integers only: every comparison is ``array_equal``, for ``sums`` and for ``err``.

Shapes: 37 x 53 (smaller than one 32 x 64 tile, odd sides), 70 x 131 and 100 x 200 (3 x 3 and 4 x 4 tiles, the last ones
ragged).  Grids: 7.3-pixel cells from a negative fractional origin (they overhang all four sides and their edges cross the
tile borders at rows 32 / 64 / 96 and columns 64 / 128 / 192 on both axes), cells of exactly one pixel at a fractional
origin (every pixel meets 2 x 2 cells; with Z * K = 9 or 64 a tile's cells do not fit the workgroup's bins: the path of
direct global atomics; with Z * K = 2 the 37 x 53 raster's 38 x 54 cells still fit: the LDS path with many cells), one cell
larger than the raster, and uneven cells.  Maps: one class only (every lane of a tile adds to the same bin), 97 % one
class, and uniform."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from deadtrees_amd.deployment.cover import CoverGrid, GridConfig, cover_grid, cover_grid_host  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(37, 53), (70, 131), (100, 200)]
KZ = [(2, 1), (3, 3), (8, 8)]
GRIDS = {
    "7.3 px, overhanging": GridConfig(7.3, (-2.61, -11.27)),
    "1.0 px": GridConfig(1.0, (0.3, -0.4)),
    "one cell": GridConfig(300.0, (-40.5, -20.25)),
    "uneven": GridConfig((5.5, 12.25), (1.3, -3.7)),
}
KINDS = ("single", "skewed", "uniform")


@functools.lru_cache(maxsize=None)
def _maps(h, w, K, Z, kind):
    rng = np.random.default_rng(7 * h + w + 100 * K + 10 * Z + len(kind))
    if kind == "single":
        c = np.full((h, w), K - 1, np.uint8)
    elif kind == "skewed":
        c = np.where(rng.random((h, w)) < 0.97, 0, rng.integers(1, K, (h, w))).astype(np.uint8)
    else:
        c = rng.integers(0, K, (h, w), dtype=np.uint8)
    z = rng.integers(0, Z, (h, w), dtype=np.uint8)
    c.setflags(write=False)
    z.setflags(write=False)
    return c, z


@functools.lru_cache(maxsize=None)
def _reference(h, w, K, Z, kind, grid):
    """(yq, xq, host sums, host sums without zones): computed once per case"""
    c, z = _maps(h, w, K, Z, kind)
    _, yq, _, xq = GRIDS[grid].edges((h, w))
    sums, err = cover_grid_host(c, z, K, Z, yq, xq)
    plain, err1 = cover_grid_host(c, None, K, 1, yq, xq)
    assert err == 0 and err1 == 0
    for a in (yq, xq, sums, plain):
        a.setflags(write=False)
    return yq, xq, sums, plain


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                                   # a copy: the cached maps are read-only


# ---------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("K,Z", KZ)
@pytest.mark.parametrize("h,w", SHAPES)
def test_kernel_against_the_host_sums(h, w, K, Z):
    from deadtrees_amd import ops
    for grid in GRIDS:
        for kind in KINDS:
            c, z = _maps(h, w, K, Z, kind)
            yq, xq, want, plain = _reference(h, w, K, Z, kind, grid)
            sums, err = ops.cover_grid(_dev(c), _dev(z), K, Z, yq, xq)
            assert sums.dtype == torch.int64 and tuple(sums.shape) == (len(yq) - 1, len(xq) - 1, Z, K)
            assert err.dtype == torch.int32 and tuple(err.shape) == (1,)
            got = sums.cpu().numpy()
            assert np.array_equal(got, want), (grid, kind)
            assert int(got.sum()) == 65536 * h * w and int(err) == 0, (grid, kind)   # every grid here covers the raster
            if kind != "uniform":
                got, err = ops.cover_grid(_dev(c), None, K, 1, yq, xq)             # zones=None: every pixel is zone 0
                assert np.array_equal(got.cpu().numpy(), plain) and int(err) == 0, (grid, kind)


def test_tables_that_cover_a_part_of_the_raster():
    from deadtrees_amd import ops
    c, z = _maps(70, 131, 3, 3, "uniform")
    for yq, xq in ((np.array([300, 700, 9000]), np.array([-100, 256, 17000, 20000])),
                   (np.array([256 * 70 - 3, 256 * 71]), np.array([256 * 131 - 1, 256 * 140])),         # the last corner
                   (np.array([-5000, -1000]), np.array([0, 256])),                                     # above the raster
                   (np.array([256 * 70, 256 * 90]), np.array([0, 256 * 131]))):                        # below it
        sums, err = ops.cover_grid(_dev(c), _dev(z), 3, 3, yq, xq)
        want, _ = cover_grid_host(c, z, 3, 3, yq, xq)
        assert np.array_equal(sums.cpu().numpy(), want) and int(err) == 0


def test_crops_stacked_members_and_misaligned_views():
    from deadtrees_amd import ops
    c, z = _maps(100, 200, 3, 3, "skewed")
    dc, dz = _dev(c), _dev(z)
    grid = GRIDS["7.3 px, overhanging"]
    for crop in ((slice(7, 91), slice(3, 190, 2)),                                 # non-contiguous: made contiguous
                 (slice(7, 91), slice(5, 132)),                                    # a window: non-contiguous rows
                 (slice(7, 44), slice(None))):                                     # full rows: contiguous at offset 7 * 200
        cc, zc = c[crop], z[crop]
        _, yq, _, xq = grid.edges(cc.shape)
        got, err = ops.cover_grid(dc[crop], dz[crop], 3, 3, yq, xq)
        assert np.array_equal(got.cpu().numpy(), cover_grid_host(cc, zc, 3, 3, yq, xq)[0]) and int(err) == 0, crop
    # member m of a stacked [3, 37, 53] tensor: a contiguous view at an odd byte offset
    stack = np.stack([_maps(37, 53, 3, 3, kind)[0] for kind in KINDS])
    zone = _maps(37, 53, 3, 3, "uniform")[1]
    ds, dzone = _dev(stack), _dev(zone)
    _, yq, _, xq = grid.edges((37, 53))
    for m in range(3):
        assert ds[m].is_contiguous() and ds[m].data_ptr() % 2 == m % 2
        got, err = ops.cover_grid(ds[m], dzone, 3, 3, yq, xq)
        assert np.array_equal(got.cpu().numpy(), cover_grid_host(stack[m], zone, 3, 3, yq, xq)[0]) and int(err) == 0, m
    # both maps at their own offsets inside buffers of out-of-range bytes: nothing outside the views is read into a sum
    c, z = _maps(37, 53, 3, 3, "skewed")
    want = cover_grid_host(c, z, 3, 3, yq, xq)[0]
    for a, za in ((1, 8), (3, 5), (8, 0), (13, 15)):
        cbuf = torch.full((37 * 53 + 64,), 200, dtype=torch.uint8, device=DEV)
        zbuf = torch.full((37 * 53 + 64,), 200, dtype=torch.uint8, device=DEV)
        cbuf[a:a + 37 * 53] = _dev(c).view(-1)
        zbuf[za:za + 37 * 53] = _dev(z).view(-1)
        cv, zv = cbuf[a:a + 37 * 53].view(37, 53), zbuf[za:za + 37 * 53].view(37, 53)
        assert cv.is_contiguous() and cv.data_ptr() % 16 == a and zv.data_ptr() % 16 == za
        got, err = ops.cover_grid(cv, zv, 3, 3, yq, xq)
        assert np.array_equal(got.cpu().numpy(), want) and int(err) == 0, (a, za)


def test_sums_add_up_over_two_calls():
    from deadtrees_amd import ops
    c1, z1 = _maps(70, 131, 3, 3, "skewed")
    c2, z2 = _maps(70, 131, 3, 3, "uniform")
    yq, xq, want1, _ = _reference(70, 131, 3, 3, "skewed", "uneven")
    sums, err = ops.cover_grid(_dev(c1), _dev(z1), 3, 3, yq, xq)
    back, err_back = ops.cover_grid(_dev(c2), _dev(z2), 3, 3, yq, xq, sums=sums, err=err)
    assert back is sums and err_back is err
    assert np.array_equal(sums.cpu().numpy(), want1 + _reference(70, 131, 3, 3, "uniform", "uneven")[2]) and int(err) == 0


@pytest.mark.parametrize("grid", ["7.3 px, overhanging", "1.0 px"])
@pytest.mark.parametrize("what,flag", [("class K", 1), ("class 255", 1), ("zone Z", 2), ("both", 3)])
def test_values_out_of_range_set_the_flag_and_enter_no_sum(what, flag, grid):
    from deadtrees_amd import ops
    K, Z, h, w = 3, 3, 70, 131
    c, z = (a.copy() for a in _maps(h, w, K, Z, "skewed"))
    where = (np.array([0, 0, 31, 32, 69, 69]), np.array([0, 17, 63, 64, 129, 130]))
    if what in ("class K", "class 255"):
        c[where] = K if what == "class K" else 255
    elif what == "zone Z":
        z[where] = Z
    else:
        c[where[0][:3], where[1][:3]] = K
        z[where[0][2:], where[1][2:]] = Z                                          # pixel (31, 63) is wrong in both
    _, yq, _, xq = GRIDS[grid].edges((h, w))
    sums, err = ops.cover_grid(_dev(c), _dev(z), K, Z, yq, xq)
    want, want_err = cover_grid_host(c, z, K, Z, yq, xq)
    assert int(err) == flag == want_err
    got = sums.cpu().numpy()
    assert np.array_equal(got, want) and int(got.sum()) == 65536 * (h * w - 6)     # exactly those pixels are missing


def test_argument_errors_are_raised_on_the_host_before_any_launch():
    from deadtrees_amd import ops
    c, z = (_dev(a) for a in _maps(37, 53, 3, 3, "uniform"))
    _, yq, _, xq = GRIDS["uneven"].edges((37, 53))
    for K, Z, zones in ((1, 1, None), (9, 1, None), (3, 9, z), (3, 0, z), (3, 2, None)):
        with pytest.raises(ValueError):
            ops.cover_grid(c, zones, K, Z, yq, xq)
    for bad in (np.array([0, 255, 600]), np.array([0, 600, 600]), np.array([600, 0]), np.array([0]), np.array([0.0, 300.0]),
                np.array([0, 2 ** 23 + 1]), _dev(yq)):
        with pytest.raises(ValueError):
            ops.cover_grid(c, z, 3, 3, bad, xq)
        with pytest.raises(ValueError):
            ops.cover_grid(c, z, 3, 3, yq, bad)
    with pytest.raises(ValueError):
        ops.cover_grid(c, z[:, :-1], 3, 3, yq, xq)                                 # unequal shapes
    with pytest.raises(ValueError):
        ops.cover_grid(c.long(), z, 3, 3, yq, xq)
    with pytest.raises(ValueError):
        ops.cover_grid(c, z.int(), 3, 3, yq, xq)
    with pytest.raises(ValueError):
        ops.cover_grid(c.view(-1), z.view(-1), 3, 3, yq, xq)
    shape = (len(yq) - 1, len(xq) - 1, 3, 3)
    with pytest.raises(ValueError):
        ops.cover_grid(c, z, 3, 3, yq, xq, sums=torch.zeros(shape[:3] + (2,), dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        ops.cover_grid(c, z, 3, 3, yq, xq, sums=torch.zeros(shape, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError):
        ops.cover_grid(c.cpu(), z.cpu(), 3, 3, yq, xq)
    sums, err = ops.cover_grid(c, z, 3, 3, yq, xq)                                 # and nothing was left behind
    assert int(sums.sum()) == 65536 * 37 * 53 and int(err) == 0


@pytest.mark.parametrize("grid", ["7.3 px, overhanging", "1.0 px"])
def test_on_poisoned_inputs_with_the_sums_in_front_of_a_guard_band(grid):
    """tests/poison.py: three runs on guarded copies of the maps, the second and third with every allocation of the wrapper
    poisoned and guarded — ``sums`` and ``err`` come from ``torch.zeros``, so they lie between guards; a given ``sums`` is a
    guarded input.  No guard may change and the three results have the same bytes"""
    import poison
    from deadtrees_amd import ops
    h, w, K, Z = 70, 131, 3, 3
    c, z = _maps(h, w, K, Z, "skewed")
    yq, xq, want, _ = _reference(h, w, K, Z, "skewed", grid)
    flat = poison.run_three(lambda: (_dev(c), _dev(z)), lambda cc, zz: ops.cover_grid(cc, zz, K, Z, yq, xq))
    assert np.array_equal(dict(flat)["out[0]"].cpu().numpy(), want) and int(dict(flat)["out[1]"]) == 0
    given = torch.zeros(want.shape, dtype=torch.int64, device=DEV)
    flat = poison.run_three(lambda: (_dev(c), _dev(z), given), lambda cc, zz, s: ops.cover_grid(cc, zz, K, Z, yq, xq, sums=s))
    assert np.array_equal(dict(flat)["out[0]"].cpu().numpy(), want)
    torch.cuda.synchronize()


def test_the_free_function_on_arrays_and_tensors():
    c, z = _maps(100, 200, 3, 3, "skewed")
    grid = GRIDS["uneven"]
    host = cover_grid(c, 3, grid, z)
    assert cover_grid(c, 3, grid, z, device=DEV) == host and cover_grid(_dev(c), 3, grid, _dev(z)) == host
    assert cover_grid(torch.from_numpy(c.copy()), 3, grid, torch.from_numpy(z.copy())) == host
    assert cover_grid(_dev(c), 3, grid) == cover_grid(c, 3, grid)
    bad = c.copy()
    bad[50, 50] = 3
    with pytest.raises(ValueError, match="out of range"):
        cover_grid(_dev(bad), 3, grid, _dev(z))


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
E2E_GRID = GridConfig((50.0, 41.5), (-12.3, 7.77), index0=(3, -2))

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
def test_infer_tile_grid_on_every_device_path(inf, ensemble, case):
    import polygon_fixtures as pf
    from deadtrees_amd.data.polygons import PolygonSet, rasterize_host
    from deadtrees_amd.deployment.tiler import infer_tile
    raster = _raster(H, W, 31)
    model = ensemble if "vote" in case else inf
    assert model.classes == 2
    kw = dict(subtile=D, batch_size=16, device=DEV, **E2E[case])
    polys = PolygonSet.from_polygons(pf.star_polygons(4, 9, H, W, values=(1, 2)))
    if case == "soft vote":
        ensemble.vote = "soft"
    try:
        base = infer_tile(model, raster, stats=True, zones=ZONES, **kw)
        got = infer_tile(model, raster, stats=True, zones=ZONES, grid=E2E_GRID, **kw)
        burnt = infer_tile(model, raster, stats=True, zones=polys, grid=E2E_GRID, patches=True, **kw)
    finally:
        ensemble.vote = "hard"
    assert len(got) == len(base) == (3 if case == "average+probs" else 2)
    iy0, yq, ix0, xq = E2E_GRID.edges((H, W))
    for out in (got, burnt):
        assert out[0].dtype == np.uint8 and np.array_equal(out[0], base[0])        # the map of the call without grid
        grid = out[-1].grid
        assert isinstance(grid, CoverGrid) and (grid.iy0, grid.ix0) == (iy0, ix0) and (grid.K, grid.Z) == (2, 3)
        assert np.array_equal(grid.sums.sum(axis=(0, 1)), 65536 * out[-1].counts)
    assert base[-1].grid is None and np.array_equal(got[-1].counts, base[-1].counts)
    if case == "average+probs":
        assert np.array_equal(got[1], base[1])                                     # probabilities, bit for bit
    assert np.array_equal(got[-1].grid.sums, cover_grid_host(got[0], ZONES, 2, 3, yq, xq)[0])
    assert got[-1].grid.patch_count is None
    zones = rasterize_host(polys, H, W, all_touched=True)
    assert np.array_equal(burnt[-1].grid.sums, cover_grid_host(burnt[0], zones, 2, 3, yq, xq)[0])
    table = burnt[-1].patches
    assert table.n > 0 and int(burnt[-1].grid.patch_count[:, :, 1].sum()) == table.count(1)
    assert int(burnt[-1].grid.patch_count[:, :, 0].sum()) == 0
    assert int(burnt[-1].grid.patch_area.sum()) == int(table.area.sum())


def test_infer_rasters_over_two_abutting_rasters_merges_to_the_grid_of_the_mosaic(inf):
    from deadtrees_amd.deployment.tiler import infer_rasters
    whole = _raster(H, W, 31)
    cut = 193                                                                      # no cell edge: 10 m cells are 40 pixels
    t = (1000.0, 0.25, 0.0, 5000.0, 0.0, -0.25)
    transforms = {"west": t, "east": (1000.0 + 0.25 * cut,) + t[1:]}
    rasters = [("west", whole[:, :, :cut].copy()), ("east", whole[:, :, cut:].copy())]
    zones = {"west": ZONES[:, :cut], "east": ZONES[:, cut:]}
    out = dict(infer_rasters(inf, rasters, subtile=D, batch_size=16, device=DEV, skip_blank=False, stats=True, zones=zones,
                             grid=lambda key: GridConfig.from_world(transforms[key], 10.0, (3.0, -1.5))))
    mosaic = np.concatenate([out["west"][0], out["east"][0]], axis=1)
    want = cover_grid(mosaic, 2, GridConfig.from_world(t, 10.0, (3.0, -1.5)), ZONES, n_zones=3)
    merged = CoverGrid.merge([out["west"][1].grid, out["east"][1].grid])
    assert merged == want and (merged.iy0, merged.ix0) == (want.iy0, want.ix0)
    assert np.array_equal(merged.sums.sum(axis=(0, 1)), 65536 * (out["west"][1].counts + out["east"][1].counts))
