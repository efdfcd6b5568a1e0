"""Overlap-stitched tiled inference on the device (csrc/stitch.hip): the windowed gather, the average-mode blend against an
fp64 oracle, its independence of the batching, the crop-mode scatter, and ``infer_tile`` / ``infer_rasters`` end to end."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

CASES = [(300, 470, 128, 32, 2), (300, 470, 128, 64, 3), (512, 512, 256, 64, 2), (200, 330, 64, 16, 3), (64, 64, 64, 32, 2)]
ACC_TOL = 2e-6      # <= 4 terms of (weight <= 1) x softmax; a softmax is K expf of <= 2 ulp and a division: ~16 ulp of 1.0
MARGIN = 4e-6       # the class map is compared where the oracle's top two accumulators are further apart than 2 x ACC_TOL
MAX_EXCLUDED = 1e-4


def _logits(h, w, d, o, K):
    from deadtrees_amd.deployment.tiler import window_grid
    ny, nx, _ = window_grid(h, w, d, o)
    g = torch.Generator().manual_seed(1000 * h + w + d + o + K)
    return 3.0 * torch.randn((ny * nx, K, d, d), generator=g, dtype=torch.float32)


def _oracle_acc(logits_f32, h, w, d, o):
    """fp64 restatement of dt_stitch_accumulate: softmax per window pixel, ramp weight r(y) r(x), summed into the raster"""
    from deadtrees_amd.deployment.tiler import blend_ramp, window_grid
    ny, nx, s = window_grid(h, w, d, o)
    lg = logits_f32.numpy().astype(np.float64)
    e = np.exp(lg - lg.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    r = blend_ramp(d, o)
    wgt = r[:, None] * r[None, :]
    acc = np.zeros((lg.shape[1], (ny - 1) * s + d, (nx - 1) * s + d))
    for k in range(ny * nx):
        i, j = divmod(k, nx)
        acc[:, i * s:i * s + d, j * s:j * s + d] += wgt * p[k]
    return acc[:, :h, :w]


def _accumulate(logits_dev, h, w, o, batch):
    from deadtrees_amd import ops
    acc = torch.zeros((logits_dev.shape[1], h, w), dtype=torch.float32, device=DEV)
    for j in range(0, logits_dev.shape[0], batch):
        ops.stitch_accumulate(logits_dev[j:j + batch], acc, o, j)
    return acc


@pytest.mark.parametrize("h,w,d,o,K", CASES)
def test_window_gather_is_the_block_gather_at_stride_d_and_a_numpy_slice_below(h, w, d, o, K):
    """dt_window_normalize_u8: overlap 0 is bit-identical to dt_split_normalize_u8; with overlap every window is the
    [i*s : i*s+d, j*s : j*s+d] slice of the zero-padded raster through val_transform (the existing gather test's pattern)"""
    from deadtrees_amd import ops
    from deadtrees_amd.data.deadtreedata import val_transform
    from deadtrees_amd.data.synthetic import MEAN, STD
    from deadtrees_amd.deployment.tiler import window_grid
    rng = np.random.default_rng(h + w + o)
    raster = rng.integers(0, 256, (4, h, w), dtype=np.uint8)
    dev_r = torch.from_numpy(raster).to(DEV)
    nby, nbx, _ = window_grid(h, w, d, 0)
    assert torch.equal(ops.window_normalize_u8(dev_r, d, 0, 0, nby * nbx, MEAN, STD, 3),
                       ops.split_normalize_u8(dev_r, d, 0, nby * nbx, MEAN, STD, 3))
    ny, nx, s = window_grid(h, w, d, o)
    padded = np.zeros((4, (ny - 1) * s + d, (nx - 1) * s + d), np.uint8)
    padded[:, :h, :w] = raster
    wins = [padded[:, i * s:i * s + d, j * s:j * s + d] for i in range(ny) for j in range(nx)]
    want = torch.stack([val_transform(image=b.transpose(1, 2, 0))["image"][:3] for b in wins])       # [n,3,d,d] f32
    got = ops.window_normalize_u8(dev_r, d, o, 0, ny * nx, MEAN, STD, 3).cpu().permute(0, 3, 1, 2)
    assert torch.equal(got, want)
    if ny * nx > 2:
        part = ops.window_normalize_u8(dev_r, d, o, 1, ny * nx - 2, MEAN, STD, 3).cpu().permute(0, 3, 1, 2)
        assert torch.equal(part, want[1:-1])
    with pytest.raises(RuntimeError):
        ops.window_normalize_u8(dev_r, d, o, 0, ny * nx + 1, MEAN, STD, 3)
    with pytest.raises(RuntimeError):
        ops.window_normalize_u8(dev_r, d, o + 1, 0, 1, MEAN, STD, 3)


@pytest.mark.parametrize("h,w,d,o,K", CASES)
def test_accumulate_and_class_map_against_fp64_oracle(h, w, d, o, K):
    """dt_stitch_accumulate within ACC_TOL (derived above, not tuned) of the fp64 restatement; the dt_stitch_finalize map is
    the oracle's argmax wherever the oracle's top-two margin exceeds MARGIN, and at most MAX_EXCLUDED of the pixels are that
    close (the oracle alone: <= 1.5e-5 on these inputs)."""
    from conftest import parity_report
    from deadtrees_amd import ops
    logits = _logits(h, w, d, o, K)
    want = _oracle_acc(logits, h, w, d, o)
    acc = _accumulate(logits.to(DEV), h, w, o, logits.shape[0])
    err = float(np.abs(acc.cpu().numpy().astype(np.float64) - want).max())
    classes = ops.stitch_finalize(acc).cpu().numpy()
    top = np.sort(want, axis=0)
    decided = (top[-1] - top[-2]) > MARGIN
    excluded = 1.0 - float(decided.mean())
    flips = int((classes != want.argmax(axis=0))[decided].sum())
    parity_report(f"[overlap stitch h{h} w{w} d{d} o{o} K{K}] accumulator max abs err vs fp64 {err:.3e} (bound {ACC_TOL:.0e}); "
                  f"class map: {flips} flips on decided pixels, excluded share {excluded:.3e} (bound {MAX_EXCLUDED:.0e})")
    assert err <= ACC_TOL, err
    assert classes.dtype == np.uint8 and classes.shape == (h, w)
    assert excluded <= MAX_EXCLUDED, excluded
    assert flips == 0, flips


@pytest.mark.parametrize("h,w,d,o,K", CASES)
def test_accumulator_and_map_do_not_depend_on_the_batching(h, w, d, o, K):
    """one thread per pixel, windows added in ascending index: bit-identical for window batches of 1, 3, 7 and all"""
    from deadtrees_amd import ops
    logits = _logits(h, w, d, o, K).to(DEV)
    ref = _accumulate(logits, h, w, o, logits.shape[0])
    ref_map = ops.stitch_finalize(ref)
    for batch in (1, 3, 7):
        acc = _accumulate(logits, h, w, o, batch)
        assert torch.equal(acc, ref), batch
        assert torch.equal(ops.stitch_finalize(acc), ref_map), batch


@pytest.mark.parametrize("h,w,d,o,K", CASES)
def test_finalize_probabilities_and_ties(h, w, d, o, K):
    from deadtrees_amd import ops
    acc = _accumulate(_logits(h, w, d, o, K).to(DEV), h, w, o, 5)
    classes, probs = ops.stitch_finalize(acc, want_probs=True)
    assert probs.dtype == torch.float32 and tuple(probs.shape) == (K, h, w)
    assert float((probs.sum(dim=0) - 1.0).abs().max()) <= 1e-6
    assert torch.equal(classes, ops.stitch_finalize(acc))                      # the map does not depend on the probs pointer
    # constructed ties: all equal -> class 0; the two highest equal -> the lower of them
    tie = torch.full((K, 8, 40), 0.25, dtype=torch.float32, device=DEV)
    assert int(ops.stitch_finalize(tie).max()) == 0
    if K > 2:
        tie[0] = 0.125
        assert bool((ops.stitch_finalize(tie) == 1).all())
        tie[K - 1] = 0.5
        assert bool((ops.stitch_finalize(tie) == K - 1).all())


def test_crop_scatter_writes_each_kept_region_once():
    """dt_stitch_classes_u8 on random uint8 maps: every raster pixel ends up with the byte of the one window whose kept
    region holds it, for any split of the windows into calls"""
    from deadtrees_amd import ops
    from deadtrees_amd.deployment.tiler import window_grid, window_keep
    for h, w, d, o, _ in CASES:
        ny, nx, s = window_grid(h, w, d, o)
        n = ny * nx
        g = torch.Generator().manual_seed(h + w + o)
        maps = torch.randint(0, 256, (n, d, d), generator=g, dtype=torch.uint8)
        want = np.zeros(((ny - 1) * s + d, (nx - 1) * s + d), np.uint8)
        for k in range(n):
            i, j = divmod(k, nx)
            (y0, y1), (x0, x1) = window_keep(i, ny, d, o), window_keep(j, nx, d, o)
            want[y0:y1, x0:x1] = maps[k].numpy()[y0 - i * s:y1 - i * s, x0 - j * s:x1 - j * s]
        dev_maps = maps.to(DEV)
        for batch in (n, 1, 3):
            out = torch.full((h, w), 255, dtype=torch.uint8, device=DEV)
            for j in range(0, n, batch):
                ops.stitch_classes(dev_maps[j:j + batch], out, o, j)
            assert np.array_equal(out.cpu().numpy(), want[:h, :w]), (h, w, d, o, batch)


@pytest.fixture(scope="module")
def inf(tmp_path_factory):
    from deadtrees_amd.deployment.inference import PyTorchInference
    from deadtrees_amd.network.segmodel import SemSegment
    from deadtrees_amd.utils.config import default_network, default_training
    from oracle.unet_ref import make_oracle
    model = SemSegment(default_network(), default_training())
    model.model.load_state_dict(make_oracle(3, 2, seed=1).state_dict())
    p = tmp_path_factory.mktemp("ckpt") / "bestmodel.ckpt"
    model.save_checkpoint(p)
    return PyTorchInference(p)


def _raster(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (4, h, w), dtype=np.uint8)


@pytest.mark.parametrize("h,w,d,o", [(300, 470, 128, 32), (200, 330, 64, 16), (100, 330, 128, 64), (64, 64, 64, 32),
                                     (256, 256, 128, 64)])
def test_infer_tile_crop_mode_is_predict_classes_on_every_kept_region(inf, h, w, d, o):
    """crop mode, bit for bit: the map of ``infer_tile(..., overlap=o, blend="crop")`` is a host assembly of
    ``predict_classes`` over the ``ops.window_normalize_u8`` windows, each keeping ``window_keep``'s region — ragged
    rasters, h < d and a single window included; no softmax, no blending arithmetic"""
    from deadtrees_amd import ops
    from deadtrees_amd.data.synthetic import MEAN, STD
    from deadtrees_amd.deployment.tiler import infer_tile, window_grid, window_keep
    raster = _raster(h, w, h + w + o)
    m = inf._model.to(DEV).eval()
    ny, nx, s = window_grid(h, w, d, o)
    x = ops.window_normalize_u8(torch.from_numpy(raster[:3].copy()).to(DEV), d, o, 0, ny * nx, MEAN, STD, 3)
    maps = m.predict_classes(x, dtype="uint8", nhwc=True).cpu().numpy()
    want = np.zeros(((ny - 1) * s + d, (nx - 1) * s + d), np.uint8)
    for k in range(ny * nx):
        i, j = divmod(k, nx)
        (y0, y1), (x0, x1) = window_keep(i, ny, d, o), window_keep(j, nx, d, o)
        want[y0:y1, x0:x1] = maps[k][y0 - i * s:y1 - i * s, x0 - j * s:x1 - j * s]
    got = infer_tile(inf, raster, subtile=d, batch_size=5, device=DEV, overlap=o, blend="crop")
    assert got.dtype == np.uint8 and got.shape == (h, w)
    assert np.array_equal(got, want[:h, :w])
    assert np.array_equal(got, infer_tile(inf, raster, subtile=d, batch_size=64, device=DEV, overlap=o))   # crop is the default


@pytest.mark.parametrize("h,w,d,o", [(300, 470, 128, 32), (100, 330, 128, 64), (512, 512, 256, 64)])
def test_infer_tile_average_mode_is_the_stitch_kernels_on_run_windows_logits(inf, h, w, d, o):
    """average mode: the map is ``stitch_finalize(stitch_accumulate(...))`` run by hand on ``run_windows(want="logits")``,
    identical for batch sizes 4 and 64; the logits are the ones the fused argmax of ``want="classes"`` is taken from; the
    returned probabilities are finalize's"""
    from deadtrees_amd import ops
    from deadtrees_amd.deployment.tiler import infer_tile, window_grid
    raster = _raster(h, w, h + w + o + 1)
    ny, nx, _ = window_grid(h, w, d, o)
    dev_r = torch.from_numpy(raster[:3].copy()).to(DEV)
    logits = inf.run_windows(dev_r, d, o, 0, ny * nx, want="logits")
    assert logits.dtype == torch.float32 and tuple(logits.shape) == (ny * nx, 2, d, d)
    classes = inf.run_windows(dev_r, d, o, 0, ny * nx, want="classes")
    assert classes.dtype == torch.uint8 and torch.equal(logits.argmax(dim=1).to(torch.uint8), classes)
    acc = ops.stitch_accumulate(logits, torch.zeros((2, h, w), dtype=torch.float32, device=DEV), o, 0)
    want_map, want_probs = ops.stitch_finalize(acc, want_probs=True)
    got4 = infer_tile(inf, raster, subtile=d, batch_size=4, device=DEV, overlap=o, blend="average")
    got64, probs = infer_tile(inf, raster, subtile=d, batch_size=64, device=DEV, overlap=o, blend="average", return_probs=True)
    assert got4.dtype == np.uint8 and got4.shape == (h, w)
    assert np.array_equal(got4, want_map.cpu().numpy()) and np.array_equal(got64, got4)
    assert probs.dtype == np.float32 and np.array_equal(probs, want_probs.cpu().numpy())
    if h * w >= 512 * 512:
        assert 0 < got4.mean() < 1                                # both classes occur: the comparison is not vacuous


def test_run_windows_bf16_and_argument_checks(inf):
    from deadtrees_amd.deployment.tiler import window_grid
    h, w, d, o = 200, 330, 64, 16
    dev_r = torch.from_numpy(_raster(h, w, 5)[:3].copy()).to(DEV)
    ny, nx, _ = window_grid(h, w, d, o)
    lg = inf.run_windows(dev_r, d, o, 2, 6, want="logits", precision="bf16")
    cl = inf.run_windows(dev_r, d, o, 2, 6, want="classes", precision="bf16")
    assert tuple(lg.shape) == (6, 2, d, d) and torch.equal(lg.argmax(dim=1).to(torch.uint8), cl)
    assert torch.equal(inf.run_windows(dev_r, d, 0, 0, 4), inf.run_blocks(dev_r, d, 0, 4))
    with pytest.raises(ValueError):
        inf.run_windows(dev_r, d, o, 0, 1, want="probs")
    with pytest.raises(RuntimeError):
        inf.run_windows(dev_r, d, o, ny * nx - 1, 2)


def test_overlap_zero_is_the_default_path(inf):
    from deadtrees_amd.deployment.tiler import infer_tile
    raster = _raster(200, 330, 9)
    base = infer_tile(inf, raster, subtile=128, batch_size=4, device=DEV)
    assert np.array_equal(infer_tile(inf, raster, subtile=128, batch_size=4, device=DEV, overlap=0), base)
    assert np.array_equal(infer_tile(inf, raster, subtile=128, batch_size=4, device=DEV, overlap=0, blend="average"), base)


def test_infer_rasters_with_overlap_skips_blank_rasters_and_shards_by_rank(inf):
    from deadtrees_amd.deployment.tiler import infer_rasters, infer_tile
    raster = _raster(200, 330, 3)
    blank = raster.copy()
    blank[0] = np.where(blank[0] > 127, 255, 0)
    queue = [("a", raster), ("blank", blank), ("c", raster[:, :128, :256])]
    for blend in ("crop", "average"):
        kw = dict(subtile=128, batch_size=4, device=DEV, overlap=32, blend=blend)
        got = dict(infer_rasters(inf, queue, **kw))
        assert list(got) == ["a", "blank", "c"] and got["blank"] is None
        assert np.array_equal(got["a"], infer_tile(inf, raster, **kw)) and got["c"].shape == (128, 256)
        assert np.array_equal(got["c"], infer_tile(inf, raster[:, :128, :256], **kw))
        assert infer_tile(inf, blank, **kw) is not None                    # the filter is opt-in on infer_tile
        assert infer_tile(inf, blank, skip_blank=True, **kw) is None
        r0 = dict(infer_rasters(inf, queue, rank=0, world=2, **kw))
        r1 = dict(infer_rasters(inf, queue, rank=1, world=2, **kw))
        assert list(r0) == ["a", "c"] and list(r1) == ["blank"] and r1["blank"] is None
        assert np.array_equal(r0["a"], got["a"]) and np.array_equal(r0["c"], got["c"])
