"""``analysis.run_device`` against ``analysis.run_host`` on handmade maps: the same ``MapAnalysis`` request goes to both, the
``RasterStats`` compare with ``==`` (counts, table, outlines, overlaps) and the maps with ``array_equal``.  No network runs:
the device runner is given the map it would get from one.  Shapes: one pixel; one row of ``ops.OVERLAP_CHUNK`` + 1 pixels
(a chunk border of the outline and of the overlap kernels); 37 x 53 (an odd pixel count); 97 x 131, the two years of
tests/test_analysis_host.py — 600 patches with holes among them, a sieve that keeps 132 of 1007, every class in every zone.
The bad requests are in the host file: nothing here is refused."""
import numpy as np
import pytest
import torch

import test_analysis_host as th
import test_overlaps_gpu as tov
from deadtrees_amd.data.polygons import PolygonSet, rasterize_host
from deadtrees_amd.deployment.analysis import MapAnalysis, run_device, run_host
from deadtrees_amd.deployment.patches import PatchConfig

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = th.K
CONFIGS = [PatchConfig(8, 0), PatchConfig(4, 6)]
AGAINST_CONFIG = PatchConfig(8, 3)


def _both(result, **options):
    """the request of ``options`` through both runners: the host's ``(map, RasterStats)`` after the device's was found equal;
    neither the caller's maps nor the uploaded ``against`` plane are written"""
    request = MapAnalysis.of("test", result.shape, K, **options)
    against = options.get("against")
    keep = None if against is None or isinstance(against, PolygonSet) else against.copy()
    want_map, want = run_host(request, result)
    out = torch.from_numpy(result.copy()).to(DEV)
    planes = request.device_planes(result.shape, out.device)
    got_map, got = run_device(request, out, None, planes)
    assert got == want, options
    assert isinstance(got_map, np.ndarray) and got_map.dtype == np.uint8 and np.array_equal(got_map, want_map)
    if against is not None:
        burnt = rasterize_host(against, *result.shape, all_touched=True) if keep is None else keep
        assert planes[1].dtype == torch.uint8 and np.array_equal(planes[1].cpu().numpy(), burnt)       # sieved on a clone
        assert keep is None or np.array_equal(against, keep)
    return want_map, want


def _squares(h, w, values, n, seed):
    rng = np.random.default_rng(seed)
    return PolygonSet.from_polygons([(values[k % len(values)], th._square(rng.uniform(3, h - 3), rng.uniform(3, w - 3),
                                                                          rng.uniform(1.5, 6))) for k in range(n)])


@pytest.mark.parametrize("config", CONFIGS, ids=repr)
def test_two_years_every_combination(config):
    a, b, zones = th.two_years()
    assert np.array_equal(a, tov._blobs(97, 131, 21, 0.03))
    _, plain = _both(b, patches=config)
    _, outlined = _both(b, patches=config, outlines=True)
    got_map, full = _both(b, zones=zones, patches=config, outlines=True, against=a, against_patches=AGAINST_CONFIG)
    # worth comparing: patches, holes, pairs, every class in every zone, a sieve that removes and keeps
    assert plain.patches.n > 0 and plain.outlines is None and plain.overlaps is None
    assert len(outlined.outlines.ring_polygon) > outlined.patches.n == plain.patches.n
    assert len(full.overlaps) > 0 and full.counts.shape == (3, K) and (full.counts > 0).all()
    assert full.patches == plain.patches and np.array_equal(full.outlines.xy, outlined.outlines.xy)
    unsieved = run_host(MapAnalysis.of("test", b.shape, K, patches=PatchConfig(config.connectivity)), b)[1].patches.n
    assert (plain.patches.n < unsieved and not np.array_equal(got_map, b)) if config.sieves else np.array_equal(got_map, b)
    # counts alone, and counts by zone without patches: the map leaves by the plain copy
    _both(b)
    _both(b, zones=zones, n_zones=5)


@pytest.mark.parametrize("config", CONFIGS, ids=repr)
@pytest.mark.parametrize("zones_as,against_as", [("polygons", "array"), ("array", "polygons"), ("polygons", "polygons")])
def test_two_years_zones_and_against_as_polygons(config, zones_as, against_as):
    a, b, zones = th.two_years()
    if zones_as == "polygons":
        zones = _squares(97, 131, (1, 2), 12, 5)
    if against_as == "polygons":
        a = _squares(97, 131, (1, 2), 25, 7)
    _, full = _both(b, zones=zones, patches=config, outlines=True, against=a, against_patches=AGAINST_CONFIG)
    assert len(full.overlaps) > 0 and full.overlaps.table_a.n > 0 and full.counts.shape == (3, K)
    assert (full.counts.sum(axis=1) > 0).all()


@pytest.mark.parametrize("config", CONFIGS, ids=repr)
def test_small_and_chunk_crossing_shapes(config):
    from deadtrees_amd import ops
    C = ops.OVERLAP_CHUNK
    assert C == ops.OUTLINE_CHUNK
    one = np.ones((1, 1), np.uint8)
    row, row_a = th.blobs(1, C + 1, 3, 0.2), th.blobs(1, C + 1, 4, 0.2)
    row[0, C - 7:] = 1                      # a patch of 8 pixels across the chunk border, kept by both configurations
    row_a[0, C - 2:] = 2
    odd, odd_a = th.blobs(37, 53, 1, 0.1), th.blobs(37, 53, 11, 0.1)
    odd[-1, -3:] = 1                        # the last pixels of an odd pixel count
    for result, against in ((one, one), (one, np.zeros((1, 1), np.uint8)), (row, row_a), (odd, odd_a)):
        h, w = result.shape
        zones = (np.arange(w)[None, :] * 3 // w + np.zeros((h, 1), int)).astype(np.uint8)
        _both(result, patches=config)
        _both(result, patches=config, outlines=True)
        _, full = _both(result, zones=zones, n_zones=3, patches=config, outlines=True, against=against,
                        against_patches=AGAINST_CONFIG)
        assert full.counts.shape == (3, K) and int(full.counts.sum()) == h * w
        if w > 1:
            assert full.patches.n > 0 and len(full.overlaps) > 0
