"""``ops.patch_depth2`` and ``ops.split_patches`` (csrc/crowns.hip) against ``depth2_host`` / ``split_patches_host`` by
``array_equal`` on every output, and ``infer_tile`` with ``crowns`` end to end against ``analysis.run_host``.  The host functions
are pinned to scalar restatements in tests/test_crowns_host.py.  Shapes: (1, 1), (1, 67), (70, 149) and (97, 260) — odd widths
for the 16-byte accesses of the growth kernel, several 32 x 64 labeller tiles, two column segments of 64 rows, a row pass that
is narrower than its window.  Integers only: every comparison is exact."""
import numpy as np
import pytest
import torch

import test_crowns_host as tch
from deadtrees_amd import ops
from deadtrees_amd.deployment.analysis import MapAnalysis, run_host
from deadtrees_amd.deployment.crowns import (CrownConfig, crown_depths_host, depth2_host, split_patches,
                                             split_patches_host)
from deadtrees_amd.deployment.patches import PatchConfig, label_patches_host, measure_patches_host

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _maps():
    """name -> (uint8 map, K)"""
    yy, xx = np.mgrid[0:97, 0:260]
    bar = np.zeros((70, 149), np.uint8)
    bar[20:31, 2:13] = 1
    bar[25, 13:113] = 1                                           # a lobe of 100 pixels: more than three groups of rounds
    row = np.zeros((1, 67), np.uint8)
    row[0, 3:30], row[0, 30:41], row[0, 50:67] = 1, 2, 1
    return {
        "cover": (tch.random_map(97, 260, 3, 5, cover=2.0, grow=4), 3),           # 253 patches, 383 crowns at E = 4, 328 at 9
        "cover, odd": (tch.random_map(70, 149, 3, 6, cover=2.0, grow=3), 3),
        "discs on a tile corner": (tch.two_discs(70, 149, ((32, 59), (32, 69))), 2),
        "lobe bar": (bar, 2),
        "checkerboard": (((yy + xx) % 2).astype(np.uint8), 2),
        "full": (np.ones((97, 260), np.uint8), 2),
        "full row": (np.full((1, 67), 2, np.uint8), 3),
        "row": (row, 3),
        "one pixel": (np.ones((1, 1), np.uint8), 2),
        "one pixel, no patch": (np.zeros((1, 1), np.uint8), 2),
    }


MAPS = _maps()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("cap2", [1, 16, 65535])
@pytest.mark.parametrize("name", sorted(MAPS))
def test_patch_depth2_equals_host(name, cap2):
    m, K = MAPS[name]
    want = depth2_host(m, K, cap2)
    depth2, err = ops.patch_depth2(_dev(m), K, cap2)
    assert depth2.dtype == torch.int32 and np.array_equal(depth2.cpu().numpy(), want) and int(err.cpu()) == 0
    if name.startswith("full"):
        assert (want == cap2).all()
    core2 = min(cap2, 4)
    depth2, core, err = ops.patch_depth2(_dev(m), K, cap2, core2=core2)
    assert np.array_equal(depth2.cpu().numpy(), want) and int(err.cpu()) == 0
    assert core.dtype == torch.uint8 and np.array_equal(core.cpu().numpy(), np.where(want >= core2, m, 0))


def test_patch_depth2_flags_a_class_out_of_range_and_checks_its_arguments():
    m = MAPS["row"][0]
    depth2, err = ops.patch_depth2(_dev(m), 2, 65535)
    assert int(err.cpu()) == 1
    want = depth2_host(np.where(m < 2, m, 0).astype(np.uint8), 2)      # the class counts as another one, and has no depth
    assert np.array_equal(depth2.cpu().numpy()[m < 2], want[m < 2]) and (depth2.cpu().numpy()[m >= 2] == 0).all()
    with pytest.raises(RuntimeError, match="patch_depth2: cap2"):
        ops.patch_depth2(_dev(m), 3, 0)
    with pytest.raises(RuntimeError, match="patch_depth2: core2=9 above cap2=4"):
        ops.patch_depth2(_dev(m), 3, 4, core2=9)
    with pytest.raises(RuntimeError, match="patch_depth2: classes must be uint8"):
        ops.patch_depth2(_dev(m.astype(np.int32)), 3)
    with pytest.raises(RuntimeError, match="split_patches: config must be a CrownConfig"):
        ops.split_patches(_dev(m), _dev(label_patches_host(m, 3, 8)), 3, 8, 9)
    with pytest.raises(RuntimeError, match="split_patches: connectivity"):
        ops.split_patches(_dev(m), _dev(label_patches_host(m, 3, 8)), 3, 6, CrownConfig(4))


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", sorted(MAPS))
def test_split_patches_equals_host(name, connectivity):
    m, K = MAPS[name]
    lp = label_patches_host(m, K, connectivity)
    classes, labels = _dev(m), _dev(lp)
    for E in (1, 4, 9, 25, 65535):
        for max_rounds in (0, 1, 3, 256):
            config = CrownConfig(E, max_rounds)
            want, want_depth2, converged, rounds = split_patches_host(m, lp, K, connectivity, config, return_rounds=True)
            crowns, depth2, crown_depth, flags = ops.split_patches(classes, labels, K, connectivity, config)
            what = (name, connectivity, E, max_rounds)
            assert crowns.dtype == torch.int32 and np.array_equal(crowns.cpu().numpy(), want), what
            assert np.array_equal(depth2.cpu().numpy(), want_depth2), what
            assert np.array_equal(crown_depth.cpu().numpy(), crown_depths_host(want, want_depth2)), what
            assert flags.cpu().tolist() == [0, int(not converged), rounds], what
            if E == 1:
                assert np.array_equal(want, lp) and converged and rounds == 0
    assert np.array_equal(classes.cpu().numpy(), m) and np.array_equal(labels.cpu().numpy(), lp)      # neither is written


def test_the_rounds_stop_early_and_run_over_several_groups():
    m, K = MAPS["lobe bar"]
    lp = label_patches_host(m, K, 8)
    G = ops.CROWN_ROUND_GROUP
    assert G == 8
    # two rounds fill the square around its core, then the lobe grows by one pixel a round: 102 rounds
    for max_rounds, rounds, converged in ((256, 102, True), (102, 102, True), (101, 101, False), (3 * G, 3 * G, False),
                                          (3 * G + 1, 3 * G + 1, False)):
        flags = ops.split_patches(_dev(m), _dev(lp), K, 8, CrownConfig(9, max_rounds))[3].cpu().tolist()
        assert flags == [0, int(not converged), rounds], max_rounds
        assert split_patches_host(m, lp, K, 8, CrownConfig(9, max_rounds), return_rounds=True)[2:] == (converged, rounds)


def test_known_answers_on_the_device():
    bar = tch.lobe_bar()
    crowns, split = split_patches(_dev(bar), 2, CrownConfig(9, 2))
    assert crowns.is_cuda and split.table.root.tolist() == [98, 349] and split.table.area.tolist() == [121, 33]
    assert not split.converged and split.parent_root.tolist() == [98, 98] and split.depth2.tolist() == [36, 1]
    host_crowns, host_split = split_patches(bar, 2, CrownConfig(9, 2))
    assert np.array_equal(crowns.cpu().numpy(), host_crowns) and split == host_split
    crowns, split = split_patches(_dev(bar), 2, CrownConfig(9, 40))
    assert split.table.root.tolist() == [98] and split.table.area.tolist() == [154] and split.converged
    discs = tch.two_discs()
    for E, n in ((16, 1), (25, 2), (36, 2), (49, 1)):
        crowns, split = split_patches(_dev(discs), 2, CrownConfig(E, 12))
        assert split.n == n and split.converged and split.n_patches == 1
        if E == 25:
            assert split.table.root.tolist() == [228, 238] and split.table.area.tolist() == [112, 105]
            assert split.depth2.tolist() == [37, 37]


def test_a_view_at_an_odd_offset_is_read_where_it_can_be():
    m, K = MAPS["cover, odd"]
    lp = label_patches_host(m, K, 8)
    padded = torch.zeros(m.size + 3, dtype=torch.uint8, device=DEV)
    padded[3:] = _dev(m).view(-1)
    view = padded[3:].view(m.shape)                               # contiguous, 3 bytes past an aligned address
    want = split_patches_host(m, lp, K, 8, CrownConfig(4))[0]
    assert np.array_equal(ops.split_patches(view, _dev(lp), K, 8, CrownConfig(4))[0].cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------- end to end
H, W, D = 160, 224, 64


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from deadtrees_amd.deployment.inference import PyTorchInference
    from deadtrees_amd.network.segmodel import SemSegment
    from deadtrees_amd.utils.config import default_network, default_training
    from oracle.unet_ref import make_oracle
    net = SemSegment(default_network(in_channels=4), default_training())
    net.model.load_state_dict(make_oracle(4, 2, seed=3).state_dict())
    file = tmp_path_factory.mktemp("ckpt") / "bestmodel.ckpt"
    net.save_checkpoint(file)
    return PyTorchInference(file)


@pytest.mark.parametrize("path", ["block", "average"])
def test_infer_tile_end_to_end(model, path):
    from deadtrees_amd.deployment.tiler import infer_tile
    raster = np.random.default_rng(31).integers(0, 256, (4, H, W), dtype=np.uint8)
    against = tch.random_map(H, W, 2, 12, cover=1.0, grow=3)
    options = dict(stats=True, patches=PatchConfig(min_pixels=4), outlines=True, against=against, gaps=True, attributes=True)
    crowned = dict(crowns=CrownConfig(9), against_crowns=CrownConfig(9))
    kw = dict(subtile=D, device=DEV, batch_size=5, **(dict(overlap=16, blend="average") if path == "average" else {}))
    plain_map, plain = infer_tile(model, raster, **kw, **options)
    got_map, got = infer_tile(model, raster, **kw, **options, **crowned)
    assert np.array_equal(got_map, plain_map) and np.array_equal(got.counts, plain.counts)
    want_map, want = run_host(MapAnalysis.of("infer_tile", (H, W), 2, raster=raster, **options, **crowned),
                              got_map, raster=raster)
    assert np.array_equal(want_map, got_map) and got == want and repr(got) == repr(want)
    assert got.crowns is not None and got.crowns.n == got.patches.n >= plain.patches.n == got.crowns.n_patches
    assert got.overlaps.table_a.n > plain.overlaps.table_a.n      # the blobs of `against` have necks at E = 9
    # without the options: today's result
    today_map, today = run_host(MapAnalysis.of("infer_tile", (H, W), 2, raster=raster, **options), plain_map,
                                raster=raster)
    assert np.array_equal(today_map, plain_map) and plain == today and repr(plain) == repr(today) and plain.crowns is None
    table = measure_patches_host(label_patches_host(plain_map, 2, 8), plain_map)
    assert plain.patches == table
