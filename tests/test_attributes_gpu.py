"""``ops.patch_attributes`` (csrc/attributes.hip) against ``attribute_tables_host`` by ``array_equal`` on both tables,
``analysis.run_device`` against ``analysis.run_host`` with the ``attributes`` option, and ``infer_tile`` end to end.  The host
function is pinned to a plain Python loop in tests/test_attributes_host.py.  Shapes: one pixel with and without a patch; one
row of ``ops.ATTRIBUTE_SPAN * 64 + 1`` pixels as a single patch (the carry across a wave's span) and one of four spans + 1
(across a workgroup); 37 x 53 and 97 x 131 at both connectivities and with a sieve (widths that are no multiple of 64: runs
wrap row ends); a 64 x 64 checkerboard under 4-connectivity (every lane heads a run); 300 x 300 of all-255 pixels as one
patch (sums above 2^32); a map without patches.  Integers only: every comparison is exact."""
import numpy as np
import pytest
import torch

import test_analysis_gpu as tag
import test_analysis_host as th
import test_attributes_host as tah
from deadtrees_amd import ops
from deadtrees_amd.deployment.analysis import MapAnalysis, run_device, run_host
from deadtrees_amd.deployment.attributes import (AttributeConfig, attribute_tables_host, attributes_of, patch_attributes,
                                                 patch_attributes_host, table_columns)
from deadtrees_amd.deployment.patches import PatchConfig, labelled_patches_host

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = th.K


def _maps():
    """name -> (uint8 map, its PatchConfig)"""
    S = ops.ATTRIBUTE_SPAN
    yy, xx = np.mgrid[0:64, 0:64]
    odd, (_, year, _) = tah.random_case(37, 53, 1, 5)[0], th.two_years()
    return {
        "one pixel": (np.ones((1, 1), np.uint8), PatchConfig()),
        "one pixel, no patch": (np.zeros((1, 1), np.uint8), PatchConfig()),
        "span row": (np.ones((1, S * 64 + 1), np.uint8), PatchConfig()),
        "workgroup row": (np.full((1, 4 * S * 64 + 1), 2, np.uint8), PatchConfig()),
        "odd, 4": (odd, PatchConfig(4)), "odd, 8": (odd, PatchConfig(8)), "odd, sieved": (odd, PatchConfig(8, 4)),
        "year, 4 sieved": (year, PatchConfig(4, 6)), "year, 8": (year, PatchConfig(8)),
        "checkerboard": (((yy + xx) % 2).astype(np.uint8), PatchConfig(4)),
        "all 255": (np.ones((300, 300), np.uint8), PatchConfig()),
        "no patches": (np.zeros((37, 53), np.uint8), PatchConfig(4)),
    }


_CASES = {}


def _case(name):
    """(classes, labels, table, raster uint8 [8, h, w], probs) of a named map, computed once: the leading C planes of the
    raster are the C-band raster"""
    if name not in _CASES:
        m, config = _maps()[name]
        classes, labels, table = labelled_patches_host(m, K, config)
        _, raster, probs = tah.random_case(*m.shape, 8, 17)
        if name == "all 255":
            raster[...] = 255
        ys, xs = np.nonzero(classes)                             # exact 0.0 and 1.0 on pixels of THIS map
        if len(ys) >= 2:
            probs[classes[ys[0], xs[0]], ys[0], xs[0]], probs[classes[ys[-1], xs[-1]], ys[-1], xs[-1]] = 0.0, 1.0
        for a in (classes, labels, raster, probs):
            a.setflags(write=False)
        _CASES[name] = classes, labels, table, raster, probs
    return _CASES[name]


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(DEV)       # a copy: the cached arrays are read-only


def _pairs(C, count):
    return (((C - 1, 0), (0, C - 1), (C // 2, C // 2), (min(1, C - 1), C - 1)) if count else ())[:count]


@pytest.mark.parametrize("with_probs", [False, True], ids=["plain", "probs"])
@pytest.mark.parametrize("n_pairs", [0, 4])
@pytest.mark.parametrize("C", [1, 3, 4, 8])
def test_device_equals_host(C, n_pairs, with_probs):
    pairs = _pairs(C, n_pairs)
    for name in _maps():
        classes, labels, table, raster, probs = _case(name)
        raster = raster[:C]
        cp = (classes, probs) if with_probs else (None, None)
        want = attribute_tables_host(labels, table.root, raster, *cp, pairs)
        got = ops.patch_attributes(_dev(labels), table.root, _dev(raster), _dev(cp[0]), _dev(cp[1]), pairs)
        Q, M = table_columns(C, n_pairs, with_probs)
        assert got[0].dtype == np.int64 and got[0].shape == (table.n, Q) and got[1].dtype == np.int32 and got[1].shape == (table.n, M)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name
    # worth comparing: the crossing shapes are one patch, the checkerboard is all heads, the big patch needs 64 bits
    S = ops.ATTRIBUTE_SPAN
    assert _case("span row")[2].area.tolist() == [S * 64 + 1] and _case("workgroup row")[2].area.tolist() == [4 * S * 64 + 1]
    assert _case("checkerboard")[2].n == 2048 and _case("no patches")[2].n == 0 and _case("one pixel, no patch")[2].n == 0
    assert _case("odd, sieved")[2].n < _case("odd, 8")[2].n < _case("odd, 4")[2].n
    big = ops.patch_attributes(_dev(_case("all 255")[1]), [0], _dev(_case("all 255")[3][:C]))
    assert big[0][0].tolist() == [22_950_000] * C + [5_852_250_000] * C and big[1][0].tolist() == [255] * (2 * C)


def test_the_objects_agree_and_maps_go_in_on_the_device():
    classes, labels, table, raster, probs = _case("year, 4 sieved")
    config = AttributeConfig(((3, 0), (1, 2)), confidence=True)
    want = patch_attributes_host(labels, table, raster[:4], classes, probs, config)
    got = attributes_of(_dev(labels), table, _dev(raster[:4]), _dev(classes), _dev(probs), config, device=True)
    assert got == want and got.has_confidence and table.n == 132
    assert attributes_of(_dev(labels), table, _dev(raster[:3]), device=True) == patch_attributes_host(labels, table, raster[:3])
    year = th.two_years()[1]
    for args in ((_dev(year), raster[:4], K, probs), (year, _dev(raster[:4]), K, _dev(probs))):
        assert patch_attributes(*args, PatchConfig(4, 6), config, device=DEV) == want
    assert patch_attributes(_dev(year), _dev(raster[:4]), K, None, PatchConfig(4, 6)) == patch_attributes_host(labels, table, raster[:4])
    polys = tag._squares(97, 131, (1, 2), 25, 7)       # the spectra of annotated crowns
    on_host = patch_attributes(polys, raster[:4], K, probs)
    assert patch_attributes(polys, raster[:4], K, probs, device=DEV) == on_host and on_host.table.n > 10


def test_views_offsets_and_bad_arguments():
    classes, labels, table, raster, probs = _case("odd, 8")
    h, w = labels.shape
    raster, pairs = raster[:4], ((3, 0),)
    want = attribute_tables_host(labels, table.root, raster, classes, probs, pairs)
    # a raster of every second column, labels and classes at odd storage offsets, probabilities permuted from [h, w, K]
    wide = torch.zeros((4, h, 2 * w), dtype=torch.uint8, device=DEV)
    wide[:, :, ::2] = _dev(raster)
    flat = torch.zeros(h * w + 1, dtype=torch.int32, device=DEV)
    flat[1:] = _dev(labels).view(-1)
    bytes_ = torch.zeros(h * w + 3, dtype=torch.uint8, device=DEV)
    bytes_[3:] = _dev(classes).view(-1)
    hwk = _dev(probs).permute(1, 2, 0).contiguous()
    args = (flat[1:].view(h, w), torch.from_numpy(table.root.copy()).to(DEV), wide[:, :, ::2], bytes_[3:].view(h, w),
            hwk.permute(2, 0, 1))
    assert not args[2].is_contiguous() and not args[4].is_contiguous() and args[0].data_ptr() % 16 == 4
    keep = [a.clone() for a in args]
    got = ops.patch_attributes(*args, pairs)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert all(torch.equal(a, b) for a, b in zip(args, keep))                       # no input is written
    # a subset of the roots, a root without pixels, no roots at all
    sub = ops.patch_attributes(args[0], table.root[::3].copy(), args[2], indices=pairs)
    assert np.array_equal(sub[0], want[0][::3, :9]) and np.array_equal(sub[1], want[1][::3, :8])
    free = [int(np.flatnonzero(labels.ravel() == 0)[0])]
    lone = ops.patch_attributes(args[0], free, *args[2:], pairs)
    assert lone[0].tolist() == [[0] * 10] and lone[1].tolist() == [[255] * 4 + [0] * 4 + [65535]]
    none = ops.patch_attributes(args[0], np.zeros(0, np.int64), *args[2:], pairs)
    assert none[0].shape == (0, 10) and none[1].shape == (0, 9) and none[0].dtype == np.int64 and none[1].dtype == np.int32
    lab, roots, ras, cls, prb = args
    for bad, fragment in (((lab.long(), roots, ras), "int32"), ((lab[:-1], roots, ras), "raster must be"),
                          ((lab, roots, ras.int()), "raster must be"), ((lab, roots, ras.cpu()), "HIP device"),
                          ((lab.cpu(), roots, ras), "HIP device"), ((lab, roots, ras[0]), "raster must be"),
                          ((lab, roots, torch.zeros((9, h, w), dtype=torch.uint8, device=DEV)), "C <= 8"),
                          ((lab, roots, ras, None, None, ((4, 0),)), "indices"), ((lab, roots, ras, None, None, ((0, 1),) * 5), "indices"),
                          ((lab, roots, ras, None, prb), "both or neither"), ((lab, roots, ras, cls, None), "both or neither"),
                          ((lab, roots, ras, cls, prb.double()), "probs must be"), ((lab, roots, ras, cls, prb[:, :-1]), "probs must be"),
                          ((lab, roots, ras, cls.int(), prb), "uint8"), ((lab, roots, ras, cls, prb[:1]), "probs must be"),
                          ((lab, roots.float(), ras), "roots")):
        with pytest.raises(RuntimeError, match=fragment):
            ops.patch_attributes(*bad)


# ---------------------------------------------------------------------------------------------- the device runner
def _both(result, raster, probs=None, **options):
    """the request of ``options`` through both runners: the host's ``RasterStats`` after the device's was found equal"""
    request = MapAnalysis.of("test", result.shape, K, raster=raster, **options)
    want_map, want = run_host(request, result, raster=raster, probs=probs)
    out = torch.from_numpy(result.copy()).to(DEV)
    got = run_device(request, out, _dev(probs), request.device_planes(result.shape, out.device), _dev(raster),
                     return_probs=False)
    assert len(got) == 2 and got[1] == want, options                               # the probabilities stay on the device
    assert got[0].dtype == np.uint8 and np.array_equal(got[0], want_map)
    return want


@pytest.mark.parametrize("name", ["odd, 8", "odd, sieved", "year, 8", "year, 4 sieved"])
def test_run_device_equals_run_host(name):
    m, config = _maps()[name]
    _, _, _, raster, probs = _case(name)
    raster = raster[:4]
    confident = AttributeConfig(((3, 0), (0, 1)), confidence=True)
    only = _both(m, raster, patches=config, attributes=True)
    assert only.attributes.indices == ((3, 0),) and only.attributes.table == only.patches and only.patches.n > 20
    assert _both(m, raster, probs, patches=config, attributes=confident).attributes.has_confidence
    if not name.startswith("year"):
        return
    against, _, zones = th.two_years()
    rest = dict(zones=zones, patches=config, outlines=True, against=against, against_patches=PatchConfig(8, 3), gaps=True,
                distances=True)
    plain = run_host(MapAnalysis.of("test", m.shape, K, **rest), m)[1]
    full = _both(m, raster, probs, attributes=confident, **rest)
    assert full.attributes == _both(m, raster, probs, patches=config, attributes=confident).attributes
    assert full != plain and full.patches == plain.patches and full.gaps == plain.gaps and full.overlaps == plain.overlaps
    assert np.array_equal(full.counts, plain.counts) and np.array_equal(full.outlines.xy, plain.outlines.xy)


# ---------------------------------------------------------------------------------------------- end to end
H, W, D = 160, 224, 64


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """{in_channels: PyTorchInference} of two small random U-Nets"""
    from deadtrees_amd.deployment.inference import PyTorchInference
    from deadtrees_amd.network.segmodel import SemSegment
    from deadtrees_amd.utils.config import default_network, default_training
    from oracle.unet_ref import make_oracle
    out = {}
    for channels in (4, 3):
        model = SemSegment(default_network(in_channels=channels), default_training())
        model.model.load_state_dict(make_oracle(channels, 2, seed=3).state_dict())
        file = tmp_path_factory.mktemp(f"ckpt{channels}") / "bestmodel.ckpt"
        model.save_checkpoint(file)
        out[channels] = PyTorchInference(file)
    return out


def _host_attributes(class_map, raster, probs, config, attributes):
    sieved, labels, table = labelled_patches_host(class_map, 2, config)
    assert np.array_equal(sieved, class_map)                     # the returned map is the sieved one
    return patch_attributes_host(labels, table, raster, class_map, probs, attributes)


@pytest.mark.parametrize("config", [PatchConfig(8), PatchConfig(4, 4)], ids=repr)
def test_infer_tile_end_to_end(models, config):
    from deadtrees_amd.deployment.tiler import infer_tile
    raster = np.random.default_rng(31).integers(0, 256, (4, H, W), dtype=np.uint8)
    inf = models[4]
    kw = dict(subtile=D, device=DEV, stats=True, patches=config, gaps=True)
    # the block path
    plain_map, plain = infer_tile(inf, raster, batch_size=5, **kw)
    got_map, got = infer_tile(inf, raster, batch_size=5, attributes=True, **kw)
    assert np.array_equal(got_map, plain_map) and plain.attributes is None and got.patches.n > 3
    assert got.patches == plain.patches and got.gaps == plain.gaps and np.array_equal(got.counts, plain.counts)
    assert got.attributes == _host_attributes(got_map, raster, None, config, AttributeConfig(((3, 0),)))
    again = infer_tile(inf, raster, batch_size=2, attributes=True, **kw)
    assert np.array_equal(again[0], got_map) and again[1] == got
    # overlap, average, confidence: the probabilities come back when they are asked for, and only then
    average = dict(overlap=16, blend="average", **kw)
    confident = AttributeConfig(confidence=True)
    plain_map, plain_probs, plain = infer_tile(inf, raster, batch_size=5, return_probs=True, **average)
    got_map, got_probs, got = infer_tile(inf, raster, batch_size=5, return_probs=True, attributes=confident, **average)
    assert np.array_equal(got_map, plain_map) and np.array_equal(got_probs, plain_probs) and got_probs.dtype == np.float32
    assert got.patches == plain.patches and got.gaps == plain.gaps and np.array_equal(got.counts, plain.counts)
    want = _host_attributes(got_map, raster, got_probs, config, AttributeConfig(((3, 0),), True))
    assert got.attributes == want and got.patches.n > 3 and (want.conf_min < want.conf_sum).any()
    again = infer_tile(inf, raster, batch_size=2, return_probs=True, attributes=confident, **average)
    assert np.array_equal(again[0], got_map) and np.array_equal(again[1], got_probs) and again[2] == got
    kept = infer_tile(inf, raster, batch_size=5, attributes=confident, **average)
    assert len(kept) == 2 and np.array_equal(kept[0], got_map) and kept[1] == got
    # an RGB model over the RGBN raster: the map of the call without the option, attributes of all four bands
    rgb_map, rgb_plain = infer_tile(models[3], raster, batch_size=5, **kw)
    got_map, got = infer_tile(models[3], raster, batch_size=5, attributes=True, **kw)
    assert np.array_equal(got_map, rgb_map) and got.patches == rgb_plain.patches
    assert got.attributes.bands == 4 and "ndvi" in got.attributes.properties() and "mean_b3" in got.attributes.properties()
    assert got.attributes == _host_attributes(got_map, raster, None, config, AttributeConfig(((3, 0),)))
