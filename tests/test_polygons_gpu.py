"""Polygon rasterisation on the device: ``dt_rasterize_polygons_u8`` (csrc/polygons.hip) through ``ops.rasterize_polygons``
/ ``data.polygons.rasterize`` against ``rasterize_host`` (itself pinned to a scalar restatement of the rule and to the known
answers in tests/test_polygons_host.py), and the two places that burn on the device instead of uploading a plane:
``DevicePool.from_rasters`` and ``infer_tile(..., stats=True, zones=PolygonSet)``.  Integers only: every comparison is
``torch.equal`` / ``array_equal``.

Shapes: 1 x 1; 33 x 65, one pixel over the kernel's 32 x 64 tile in each axis (four workgroups, three of them ragged); 70 x
150 (3 x 3 tiles, ragged on both sides, an odd row pitch); 256 x 256 (32 tiles).  Sets (tests/polygon_fixtures.py): 60 star
polygons with values 1..3, holes, some reaching outside; 400 small polygons packed over one tile (the kernel's polygon list
takes 256 at a time); one ring of 3000 vertices with a hole (its edge list takes 256 at a time); the four known answers.
The conditions that keep the comparison from being vacuous are asserted on the HOST result: zeros between 10 % and 90 % of
the pixels, every value present, the two modes different.  A single pixel cannot meet them (it is all zeros or none): at 1 x
1 the comparison alone is made."""
import functools

import numpy as np
import pytest
import torch

from polygon_fixtures import KNOWN, fixture, star_polygons

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 1), (33, 65), (70, 150), (256, 256)]
SETS = ["stars", "packed", "ring"]


@functools.lru_cache(maxsize=None)
def _host(name, h, w, all_touched):
    from deadtrees_amd.data.polygons import rasterize_host
    out = rasterize_host(fixture(name, h, w), h, w, all_touched)
    out.setflags(write=False)
    return out


def _ps(polys):
    from deadtrees_amd.data.polygons import PolygonSet
    return PolygonSet.from_polygons(polys)


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_equals_host(shape, name):
    from deadtrees_amd.data.polygons import rasterize
    h, w = shape
    polys = fixture(name, h, w)
    touched, centre = _host(name, h, w, True), _host(name, h, w, False)
    if h * w > 1:
        zeros = np.count_nonzero(touched == 0) / (h * w)
        print(f"{name} {h}x{w}: {len(polys)} polygons, zeros {zeros:.3f}, touch-only {np.count_nonzero(touched != centre)}")
        assert 0.1 < zeros < 0.9
        assert set(np.unique(touched)) == {0, 1, 2, 3} and set(np.unique(centre)) == {0, 1, 2, 3}
        assert not np.array_equal(touched, centre)
    for mode, want in ((True, touched), (False, centre)):
        got = rasterize(polys, (h, w), device=DEV, all_touched=mode)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (h, w) and got.is_cuda
        assert torch.equal(got.cpu(), torch.from_numpy(want.copy())), (name, shape, mode)


@pytest.mark.parametrize("k", range(len(KNOWN)), ids=[k[0] for k in KNOWN])
def test_known_answers_on_the_device(k):
    from deadtrees_amd.data.polygons import rasterize, rasterize_host
    _, polys, (h, w), n_touched, n_centre = KNOWN[k]
    ps = _ps(polys)
    for mode, count in ((True, n_touched), (False, n_centre)):
        got = rasterize(ps, (h, w), device=DEV, all_touched=mode).cpu().numpy()
        assert np.array_equal(got, rasterize_host(ps, h, w, mode))
        if count is not None:
            assert np.count_nonzero(got) == count


def test_out_as_a_view_into_a_larger_buffer():
    """the plane is written where it lies, at any byte offset, and no byte around it is touched"""
    from deadtrees_amd.data.polygons import rasterize
    h, w = 70, 150
    polys, want = fixture("stars", h, w), torch.from_numpy(_host("stars", h, w, True).copy())
    for lead in (0, 1, 5, 16, 77):
        buf = torch.full((lead + h * w + 300,), 200, dtype=torch.uint8, device=DEV)
        view = buf[lead:lead + h * w].view(h, w)
        back = rasterize(polys, (h, w), out=view)
        assert back.data_ptr() == view.data_ptr()
        host = buf.cpu()
        assert torch.equal(host[lead:lead + h * w].view(h, w), want), lead
        assert bool((host[:lead] == 200).all()) and bool((host[lead + h * w:] == 200).all()), lead


def test_empty_sets_and_argument_checks():
    from deadtrees_amd import ops
    from deadtrees_amd.data.polygons import rasterize
    out = torch.full((40, 70), 9, dtype=torch.uint8, device=DEV)
    assert not bool(rasterize(_ps([]), (40, 70), out=out).any())                    # zeros are written too
    assert not bool(rasterize(_ps([(1, [(100, 100), (120, 100), (120, 130)])]), (40, 70), device=DEV).any())
    edges, table = (torch.from_numpy(t.copy()).to(DEV) for t in fixture("stars", 33, 65).tables())
    assert torch.equal(ops.rasterize_polygons(edges, table, (33, 65)).cpu(), torch.from_numpy(_host("stars", 33, 65, True).copy()))
    with pytest.raises(RuntimeError):
        ops.rasterize_polygons(edges.long(), table, (33, 65))
    with pytest.raises(RuntimeError):
        ops.rasterize_polygons(edges, table[:, :7], (33, 65))
    with pytest.raises(RuntimeError):
        ops.rasterize_polygons(edges, table, (33, 65), out=torch.empty((33, 64), dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError):
        ops.rasterize_polygons(edges, table, (33, 65), out=torch.empty((65, 33), dtype=torch.uint8, device=DEV).t())
    with pytest.raises(RuntimeError):
        ops.rasterize_polygons(edges.cpu(), table.cpu(), (33, 65))
    with pytest.raises(RuntimeError):
        ops.rasterize_polygons(edges, table, (0, 65))
    with pytest.raises(RuntimeError):
        ops.rasterize_polygons(edges, table, (16385, 4))


# ---------------------------------------------------------------------------------------------- pools from rasters
def test_device_pool_from_rasters_with_polygon_mask_and_lu():
    from deadtrees_amd.data.pool import DevicePool
    from deadtrees_amd.data.polygons import rasterize_host
    from deadtrees_amd.data.rasters import pool_from_rasters
    rng = np.random.default_rng(17)
    with_polys, with_arrays = [], []
    for n, (h, w) in enumerate(((128, 128), (128, 128), (100, 117))):
        rgbn = rng.integers(0, 256, (4, h, w), dtype=np.uint8)
        rgbn[:, :32, 32:64] = 7                            # one blank sub-tile
        mask = _ps(star_polygons(40 + n, 14, h, w, values=(1, 2), radius=(0.03, 0.1)))
        lu = _ps(star_polygons(50 + n, 5, h, w, values=(1,), radius=(0.3, 0.5)))
        burnt_mask, burnt_lu = rasterize_host(mask, h, w), rasterize_host(lu, h, w)
        assert 0 < np.count_nonzero(burnt_mask) < h * w and 0 < np.count_nonzero(burnt_lu) < h * w
        # raster 0: both maps as polygons; raster 1: a polygon mask next to an uploaded lu; raster 2: ragged, mask only
        with_polys.append((f"r{n}", rgbn, mask, (lu, burnt_lu, None)[n]))
        with_arrays.append((f"r{n}", rgbn, burnt_mask, (burnt_lu, burnt_lu, None)[n]))
    kw = dict(tile_size=32, source_dim=128, device=DEV)
    for select in ("dead", "valid"):
        rec_a, rec_b = {}, {}
        a = pool_from_rasters(with_polys, select=select, record=rec_a, **kw)
        b = pool_from_rasters(with_arrays, select=select, record=rec_b, **kw)
        assert a.n == b.n > 0 and a.stats == b.stats
        assert rec_a["table"] == rec_b["table"] and rec_a["keys"] == rec_b["keys"]
        for (ca, sa), (cb, sb) in zip(rec_a["censuses"], rec_b["censuses"]):
            assert np.array_equal(ca, cb) and sa == sb
        for x, y in ((a.images, b.images), (a.masks, b.masks), (a.lu, b.lu), (a.sums, b.sums)):
            assert x.is_cuda and torch.equal(x, y)
        assert bool(a.masks.any()) and 0 < int(torch.count_nonzero(a.lu)) < a.lu.numel()
    c = DevicePool.from_rasters(with_polys, tile_size=32, source_dim=128, device=DEV)
    d = DevicePool.from_rasters(with_arrays, tile_size=32, source_dim=128, device=DEV)
    assert c.n == d.n > 0 and torch.equal(c.masks, d.masks) and torch.equal(c.lu, d.lu) and torch.equal(c.images, d.images)


# ---------------------------------------------------------------------------------------------- zones of infer_tile
@pytest.fixture(scope="module")
def inf(tmp_path_factory):
    from deadtrees_amd.deployment.inference import PyTorchInference
    from deadtrees_amd.network.segmodel import SemSegment
    from deadtrees_amd.utils.config import default_network, default_training
    from oracle.unet_ref import make_oracle
    model = SemSegment(default_network(), default_training())
    model.model.load_state_dict(make_oracle(3, 2, seed=1).state_dict())
    path = tmp_path_factory.mktemp("ckpt") / "bestmodel.ckpt"
    model.save_checkpoint(path)
    return PyTorchInference(path)


@pytest.mark.parametrize("case", ["blocks", "average"])
def test_infer_tile_with_polygon_zones(inf, case):
    from deadtrees_amd.data.polygons import rasterize_host
    from deadtrees_amd.deployment.tiler import infer_rasters, infer_tile
    h, w = 150, 200
    raster = np.random.default_rng(31).integers(0, 256, (4, h, w), dtype=np.uint8)
    zones = _ps(star_polygons(60, 9, h, w, values=(1, 2), radius=(0.15, 0.3)))
    burnt = rasterize_host(zones, h, w)
    assert set(np.unique(burnt)) == {0, 1, 2}
    kw = dict(subtile=64, batch_size=16, device=DEV, **(dict(overlap=0) if case == "blocks" else dict(overlap=16, blend="average")))
    got_map, got = infer_tile(inf, raster, stats=True, zones=zones, **kw)
    want_map, want = infer_tile(inf, raster, stats=True, zones=burnt, **kw)
    assert np.array_equal(got_map, want_map)
    assert got.counts.shape == (3, 2) and np.array_equal(got.counts, want.counts) and int(got.counts.sum()) == h * w
    five = infer_tile(inf, raster, stats=True, zones=zones, n_zones=5, **kw)[1]
    assert five.counts.shape == (5, 2) and np.array_equal(five.counts[:3], want.counts) and not five.counts[3:].any()
    with pytest.raises(ValueError):
        infer_tile(inf, raster, stats=True, zones=zones, n_zones=2, **kw)
    (_, (m, st)), = infer_rasters(inf, [("a", raster)], stats=True, zones={"a": zones}, skip_blank=False, **kw)
    assert np.array_equal(m, want_map) and np.array_equal(st.counts, want.counts)
