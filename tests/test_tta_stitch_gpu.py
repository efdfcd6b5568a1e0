"""Test-time augmentation and ensemble voting on the stitched device path (csrc/stitch.hip): the views gather, the views
accumulate against fp64 numpy oracles written here, its independence of the batching, the degenerate forms that must be
today's results bit for bit, and ``infer_tile`` / ``infer_rasters`` end to end with ``tta=`` and ensembles.

Bounds (derived, not tuned; ulp = 2^-23, one ulp of 1.0):

* ``SOFTMAX_TOL`` = 2e-6 is the bound tests/test_overlap_stitch_gpu.py derives for one model's blended softmax (``ACC_TOL``:
  <= 4 terms of weight <= 1 x a softmax of K ``expf`` of <= 2 ulp and a division, ~16 ulp of 1.0).
* accumulator, ``acc_bound(M, T)``: per model that bound plus (T - 1) ulp for the T - 1 adds of the view sum (the factor
  1/T is exact for T = 8); M models add into one accumulator that grows to M, so the <= 4 adds of model m round at
  <= m ulp / 2 instead of ulp / 2: another 2 (m - 1) ulp, M (M - 1) ulp over the models.
  ``acc_bound = M (SOFTMAX_TOL + (T - 1) ulp) + M (M - 1) ulp``: 2.8e-6 at M = 1 and 9.2e-6 at M = 3 (T = 8).
* probabilities of the network-free field test, ``PROB_TOL``: every term of a pixel is the softmax of the SAME logits, so
  the accumulator is a convex combination of equal terms and the weights (and their rounding) cancel in finalize's
  acc_k / sum acc.  Relative error of acc_k: 16 ulp (softmax) + (T - 1) / 2 (view sum) + 1/2 (weight x mean) + 3/2 (<= 3
  window adds) = 21.5 ulp; the denominator carries the same plus (K - 1) / 2 for its adds, the division 1/2: <= 45 ulp of
  a probability <= 1 = 5.4e-6 -> ``PROB_TOL = 6e-6``.  A wrong inverse view mixes pixels of a 3 N(0,1) field: errors ~ 0.1-1.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

CASES = [(200, 330, 64, 16, 3), (300, 470, 128, 32, 2), (64, 64, 64, 32, 2), (160, 160, 64, 16, 2), (100, 70, 64, 0, 3)]
D4 = tuple((f, k) for f in (0, 1) for k in range(4))
ULP = 2.0 ** -23
SOFTMAX_TOL = 2e-6
PROB_TOL = 6e-6
MAX_EXCLUDED = 5e-4


def acc_bound(M, T):
    return M * (SOFTMAX_TOL + (T - 1) * ULP) + M * (M - 1) * ULP


def _grid(h, w, d, o):
    from deadtrees_amd.deployment.tiler import window_grid
    return window_grid(h, w, d, o)


def np_view(a, flip, rot):
    """rot90^rot(flip(a)) over the last two axes"""
    f = a[..., :, ::-1] if flip == 1 else a[..., ::-1, :] if flip == 2 else a
    return np.rot90(f, rot, axes=(-2, -1))


def np_unview(a, flip, rot):
    """undo np_view: turn back, then flip back (numpy only — no use of the kernel's inverse-view rule)"""
    b = np.rot90(a, -rot, axes=(-2, -1))
    return b[..., :, ::-1] if flip == 1 else b[..., ::-1, :] if flip == 2 else b


def _softmax64(lg, axis):
    lg = lg.astype(np.float64)
    e = np.exp(lg - lg.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


@functools.lru_cache(maxsize=None)
def _model_logits(h, w, d, o, K, M):
    """the issue's inputs: M arrays [n, 8, K, d, d] fp32, drawn per model in order from one generator"""
    ny, nx, _ = _grid(h, w, d, o)
    rng = np.random.default_rng(1000 * h + w + d + o + K + M)
    return tuple((3.0 * rng.standard_normal((ny * nx, len(D4), K, d, d))).astype(np.float32) for _ in range(M))


@functools.lru_cache(maxsize=None)
def _oracle_acc(h, w, d, o, K, M, weight):
    """fp64: softmax, inverse view, mean over T, weight, sum over windows and then models -> [K, h, w]"""
    from deadtrees_amd.deployment.tiler import blend_ramp, window_keep
    ny, nx, s = _grid(h, w, d, o)
    total = np.zeros((K, (ny - 1) * s + d, (nx - 1) * s + d))
    r = blend_ramp(d, o)
    for lg in _model_logits(h, w, d, o, K, M):
        p = _softmax64(lg, axis=2)                                        # [n, T, K, d, d]
        mean = sum(np_unview(p[:, v], *view) for v, view in enumerate(D4)) / len(D4)
        acc = np.zeros_like(total)
        for k in range(ny * nx):
            i, j = divmod(k, nx)
            if weight == "ramp":
                wgt = r[:, None] * r[None, :]
            else:
                (y0, y1), (x0, x1) = window_keep(i, ny, d, o), window_keep(j, nx, d, o)
                wgt = np.zeros((d, d))
                wgt[y0 - i * s:y1 - i * s, x0 - j * s:x1 - j * s] = 1.0
            acc[:, i * s:i * s + d, j * s:j * s + d] += wgt * mean[k]
        total += acc
    total = total[:, :h, :w]
    total.setflags(write=False)
    return total


@functools.lru_cache(maxsize=None)
def _dev_logits(h, w, d, o, K, M):
    return tuple(torch.from_numpy(lg).to(DEV) for lg in _model_logits(h, w, d, o, K, M))


def _accumulate(models, h, w, o, batch, views=D4, weight="ramp"):
    """model-major: every model's windows in ascending batches of ``batch`` into one accumulator"""
    from deadtrees_amd import ops
    acc = torch.zeros((models[0].shape[2], h, w), dtype=torch.float32, device=DEV)
    for lg in models:
        for j in range(0, lg.shape[0], batch):
            ops.stitch_accumulate(lg[j:j + batch], acc, o, j, views=views, weight=weight)
    return acc


# ---------------------------------------------------------------------------------------------- 1. gather
@pytest.mark.parametrize("h,w,d,o,K", CASES)
def test_views_gather_is_a_bit_exact_permutation_of_the_plain_window(h, w, d, o, K):
    from deadtrees_amd import ops
    from deadtrees_amd.data.synthetic import MEAN, STD
    ny, nx, _ = _grid(h, w, d, o)
    n = ny * nx
    raster = np.random.default_rng(h + w + o).integers(0, 256, (4, h, w), dtype=np.uint8)
    dev_r = torch.from_numpy(raster).to(DEV)
    plain = ops.window_normalize_u8(dev_r, d, o, 0, n, MEAN, STD, 3)             # [n, d, d, 3]

    def want(flip, rot, wins):
        f = wins.flip(2) if flip == 1 else wins.flip(1) if flip == 2 else wins
        return torch.rot90(f, rot, dims=(1, 2))

    for views in (D4, tuple((2, k) for k in range(4)), ((1, 3), (0, 0), (2, 1))):
        T = len(views)
        got = ops.window_normalize_u8(dev_r, d, o, 0, n, MEAN, STD, 3, views=views)
        assert got.dtype == torch.float32 and tuple(got.shape) == (n * T, d, d, 3)
        got = got.view(n, T, d, d, 3)
        for v, (flip, rot) in enumerate(views):
            assert torch.equal(got[:, v], want(flip, rot, plain)), (flip, rot)
    if n > 2:
        part = ops.window_normalize_u8(dev_r, d, o, 1, n - 2, MEAN, STD, 3, views=D4).view(n - 2, 8, d, d, 3)
        for v, (flip, rot) in enumerate(D4):
            assert torch.equal(part[:, v], want(flip, rot, plain[1:-1])), (flip, rot)
    assert torch.equal(ops.window_normalize_u8(dev_r, d, o, 0, n, MEAN, STD, 3, views=((0, 0),)), plain)
    for bad in (((0, 4),), ((3, 0),), ((0, 0), (-1, 1)), (), D4 + ((0, 0),)):
        with pytest.raises(RuntimeError):
            ops.window_normalize_u8(dev_r, d, o, 0, 1, MEAN, STD, 3, views=bad)
    with pytest.raises(RuntimeError):
        ops.window_normalize_u8(dev_r, d, o, 0, n + 1, MEAN, STD, 3, views=D4)


# ---------------------------------------------------------------------------------------------- 2. inverse mapping
@pytest.mark.parametrize("h,w,d,o,K", CASES)
def test_views_of_one_field_blend_back_to_the_field(h, w, d, o, K):
    """network-free: logits[k, v] = view_v(F[:, window k]) of one rough random field F, so all views and all overlapping
    windows agree and the finalized probabilities are softmax(F) within PROB_TOL (derived in the header)"""
    from conftest import parity_report
    from deadtrees_amd import ops
    ny, nx, s = _grid(h, w, d, o)
    F = (3.0 * np.random.default_rng(7 * h + w + o + K).standard_normal((K, (ny - 1) * s + d, (nx - 1) * s + d))).astype(np.float32)
    wins = np.stack([F[:, i * s:i * s + d, j * s:j * s + d] for i in range(ny) for j in range(nx)])        # [n, K, d, d]
    logits = np.ascontiguousarray(np.stack([np_view(wins, *view) for view in D4], axis=1))                  # [n, 8, K, d, d]
    acc = _accumulate([torch.from_numpy(logits).to(DEV)], h, w, o, 5)
    classes, probs = ops.stitch_finalize(acc, want_probs=True)
    want = _softmax64(F, axis=0)[:, :h, :w]
    err = float(np.abs(probs.cpu().numpy().astype(np.float64) - want).max())
    parity_report(f"[tta field h{h} w{w} d{d} o{o} K{K}] probabilities max abs err vs fp64 softmax {err:.3e} "
                  f"(bound {PROB_TOL:.0e})")
    assert err <= PROB_TOL, err
    top = np.sort(want, axis=0)
    decided = (top[-1] - top[-2]) > 2 * PROB_TOL
    assert int((classes.cpu().numpy() != want.argmax(axis=0))[decided].sum()) == 0
    # keep mode: one window per pixel, the same field
    _, probs_keep = ops.stitch_finalize(_accumulate([torch.from_numpy(logits).to(DEV)], h, w, o, 5, weight="keep"),
                                        want_probs=True)
    assert float(np.abs(probs_keep.cpu().numpy().astype(np.float64) - want).max()) <= PROB_TOL


# ---------------------------------------------------------------------------------------------- 3. fp64 oracle
@pytest.mark.parametrize("weight", ["ramp", "keep"])
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("h,w,d,o,K", CASES)
def test_accumulator_and_class_map_against_fp64_oracle(h, w, d, o, K, M, weight):
    """independent logits per window, view and model, T = 8: the accumulator within acc_bound(M, 8) of the fp64 oracle; the
    finalize map is the oracle's argmax wherever the oracle's top-two margin exceeds 2 x bound, and the oracle itself has at
    most MAX_EXCLUDED of the pixels that close"""
    from conftest import parity_report
    from deadtrees_amd import ops
    bound = acc_bound(M, len(D4))
    want = _oracle_acc(h, w, d, o, K, M, weight)
    acc = _accumulate(_dev_logits(h, w, d, o, K, M), h, w, o, 4, weight=weight)
    err = float(np.abs(acc.cpu().numpy().astype(np.float64) - want).max())
    classes = ops.stitch_finalize(acc).cpu().numpy()
    top = np.sort(want, axis=0)
    decided = (top[-1] - top[-2]) > 2 * bound
    excluded = 1.0 - float(decided.mean())
    flips = int((classes != want.argmax(axis=0))[decided].sum())
    parity_report(f"[tta stitch h{h} w{w} d{d} o{o} K{K} M{M} T8 {weight}] accumulator max abs err vs fp64 {err:.3e} "
                  f"(bound {bound:.2e}); class map: {flips} flips on decided pixels, excluded share {excluded:.3e} "
                  f"(bound {MAX_EXCLUDED:.0e})")
    assert err <= bound, err
    assert classes.dtype == np.uint8 and classes.shape == (h, w)
    assert excluded <= MAX_EXCLUDED, excluded
    assert flips == 0, flips


# ---------------------------------------------------------------------------------------------- 4. batching
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("h,w,d,o,K", CASES)
def test_accumulator_and_map_do_not_depend_on_the_batching(h, w, d, o, K, M):
    """one thread per pixel; models outer, windows ascending, views ascending: bit-identical for batches of 1, 3, 7, all"""
    from deadtrees_amd import ops
    models = _dev_logits(h, w, d, o, K, M)
    for weight in ("ramp", "keep"):
        ref = _accumulate(models, h, w, o, models[0].shape[0], weight=weight)
        ref_map = ops.stitch_finalize(ref)
        for batch in (1, 3, 7):
            acc = _accumulate(models, h, w, o, batch, weight=weight)
            assert torch.equal(acc, ref), (weight, batch)
            assert torch.equal(ops.stitch_finalize(acc), ref_map), (weight, batch)


# ---------------------------------------------------------------------------------------------- 5. degenerate forms
@pytest.mark.parametrize("h,w,d,o,K", CASES)
def test_degenerate_forms_are_todays_results_bit_for_bit(h, w, d, o, K):
    from deadtrees_amd import ops
    (lg,) = _dev_logits(h, w, d, o, K, 1)
    one = lg[:, :1].contiguous()                                                   # [n, 1, K, d, d]
    n = lg.shape[0]
    # T = 1, identity, ramp == dt_stitch_accumulate, for a split into calls too
    old = torch.zeros((K, h, w), dtype=torch.float32, device=DEV)
    for j in range(0, n, 3):
        ops.stitch_accumulate(one[j:j + 3, 0], old, o, j)
    assert torch.equal(_accumulate([one], h, w, o, 3, views=((0, 0),)), old)
    assert torch.equal(_accumulate([one], h, w, o, n, views=((0, 0),)), old)
    # keep, T = 1, finalize == the crop-mode scatter of the per-window argmax; logits without (near) ties: a random
    # permutation of 0, 2, 4, .. per pixel plus noise below 0.5, so the softmax cannot round two classes together
    rng = np.random.default_rng(h + w + d + o + K)
    scores = 2.0 * np.argsort(rng.random((n, K, d, d)), axis=1) + rng.uniform(-0.4, 0.4, (n, K, d, d))
    clean = torch.from_numpy(scores.astype(np.float32)).to(DEV)
    want = ops.stitch_classes(clean.argmax(dim=1).to(torch.uint8), torch.empty((h, w), dtype=torch.uint8, device=DEV), o, 0)
    got = ops.stitch_finalize(_accumulate([clean.unsqueeze(1)], h, w, o, 4, views=((0, 0),), weight="keep"))
    assert torch.equal(got, want)
    # keep without views: plain [n, K, d, d] logits are the identity-view form bit for bit, split into calls of 3 and in one
    # call, and finalize to the same crop-mode scatter
    for batch in (3, n):
        plain = torch.zeros((K, h, w), dtype=torch.float32, device=DEV)
        for j in range(0, n, batch):
            ops.stitch_accumulate(one[j:j + batch, 0], plain, o, j, views=None, weight="keep")
        assert torch.equal(plain, _accumulate([one], h, w, o, batch, views=((0, 0),), weight="keep")), batch
    plain = torch.zeros((K, h, w), dtype=torch.float32, device=DEV)
    for j in range(0, n, 4):
        ops.stitch_accumulate(clean[j:j + 4], plain, o, j, views=None, weight="keep")
    assert torch.equal(ops.stitch_finalize(plain), want)
    if o == 0:                                                                    # block grid: both weights are 1
        assert torch.equal(_accumulate([lg], h, w, o, 4, weight="ramp"), _accumulate([lg], h, w, o, 4, weight="keep"))
    with pytest.raises(RuntimeError):
        ops.stitch_accumulate(lg, old, o, 0, views=D4, weight="max")
    with pytest.raises(RuntimeError):
        ops.stitch_accumulate(lg, old, o, 0, views=D4[:4])                          # logits carry 8 views
    with pytest.raises(RuntimeError):
        ops.stitch_accumulate(one, old, o, 0, views=((0, 5),))


# ---------------------------------------------------------------------------------------------- 6. / 7. end to end
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
    return ensemble.members[0]           # a PyTorchInference on the seed-1 checkpoint (one load serves both fixtures)


def _raster(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (4, h, w), dtype=np.uint8)


@pytest.mark.parametrize("h,w,d,o", [(200, 330, 64, 16), (160, 160, 64, 16)])
def test_infer_tile_tta_is_the_views_kernels_on_run_windows_logits(inf, h, w, d, o):
    from deadtrees_amd import ops
    from deadtrees_amd.deployment.tiler import infer_tile, tta_views
    raster = _raster(h, w, h + w + o + 2)
    ny, nx, _ = _grid(h, w, d, o)
    n = ny * nx
    dev_r = torch.from_numpy(raster[:3].copy()).to(DEV)
    views = tta_views("d4")
    logits = inf.run_windows(dev_r, d, o, 0, n, want="logits", views=views)
    assert logits.dtype == torch.float32 and tuple(logits.shape) == (n, 8, 2, d, d)
    assert torch.equal(logits[:, 0], inf.run_windows(dev_r, d, o, 0, n, want="logits"))      # view 0 is the plain window
    acc = ops.stitch_accumulate(logits, torch.zeros((2, h, w), dtype=torch.float32, device=DEV), o, 0, views=views)
    want_map, want_probs = ops.stitch_finalize(acc, want_probs=True)
    kw = dict(subtile=d, device=DEV, overlap=o, blend="average")
    got8, probs8 = infer_tile(inf, raster, batch_size=8, tta="d4", return_probs=True, **kw)
    got64, probs64 = infer_tile(inf, raster, batch_size=64, tta="d4", return_probs=True, **kw)
    assert got8.dtype == np.uint8 and got8.shape == (h, w) and probs8.dtype == np.float32 and probs8.shape == (2, h, w)
    assert np.array_equal(got8, want_map.cpu().numpy()) and np.array_equal(probs8, want_probs.cpu().numpy())
    assert np.array_equal(got64, got8) and np.array_equal(probs64, probs8)
    assert np.array_equal(infer_tile(inf, raster, batch_size=3, tta="d4", **kw), got8)         # batch below T: one window
    # the identity view alone is today's average path, map and probabilities
    base, base_probs = infer_tile(inf, raster, batch_size=8, return_probs=True, **kw)
    same, same_probs = infer_tile(inf, raster, batch_size=8, tta=[(0, 0)], return_probs=True, **kw)
    assert np.array_equal(same, base) and np.array_equal(same_probs, base_probs)
    # crop mode on the block grid runs through the keep weights
    crop = infer_tile(inf, raster, subtile=d, batch_size=16, device=DEV, overlap=0, blend="crop", tta="flips")
    assert crop.dtype == np.uint8 and crop.shape == (h, w)
    hand = torch.zeros((2, h, w), dtype=torch.float32, device=DEV)
    nb = _grid(h, w, d, 0)[0] * _grid(h, w, d, 0)[1]
    flips = tta_views("flips")
    ops.stitch_accumulate(inf.run_windows(dev_r, d, 0, 0, nb, want="logits", views=flips), hand, 0, 0, views=flips,
                          weight="keep")
    assert np.array_equal(crop, ops.stitch_finalize(hand).cpu().numpy())
    with pytest.raises(ValueError):
        inf.run_windows(dev_r, d, o, 0, 1, want="classes", views=views)
    with pytest.raises(ValueError):
        infer_tile(inf, raster, batch_size=8, tta="d4", return_probs=True, subtile=d, device=DEV, overlap=o, blend="crop")


def test_infer_rasters_forwards_tta(inf):
    from deadtrees_amd.deployment.tiler import infer_rasters, infer_tile
    raster = _raster(160, 160, 11)
    blank = raster.copy()
    blank[0] = np.where(blank[0] > 127, 255, 0)
    kw = dict(subtile=64, batch_size=16, device=DEV, overlap=16, blend="average", tta="flips")
    got = dict(infer_rasters(inf, [("a", raster), ("blank", blank)], **kw))
    assert got["blank"] is None
    assert np.array_equal(got["a"], infer_tile(inf, raster, **kw))
    plain = dict(kw, tta=None)
    assert np.array_equal(dict(infer_rasters(inf, [("a", raster)], **plain))["a"], infer_tile(inf, raster, **plain))


def test_infer_tile_ensemble_hard_and_soft_votes(ensemble, ckpts):
    from deadtrees_amd import ops
    from deadtrees_amd.deployment.inference import PyTorchEnsembleInference
    from deadtrees_amd.deployment.tiler import infer_tile, tta_views
    h, w, d = 200, 330, 64
    raster = _raster(h, w, 21)
    members = ensemble.members
    assert len(members) == 3 and ensemble.in_channels == 3 and ensemble.vote == "hard"
    kw = dict(subtile=d, batch_size=8, device=DEV)

    # hard vote, overlap 16 / crop and overlap 0 (the block path of the single models)
    for o in (16, 0):
        singles = [infer_tile(m, raster, overlap=o, blend="crop", **kw) for m in members]
        stack = torch.from_numpy(np.stack(singles))
        voted, _ = ops.ensemble_vote(stack.to(DEV), 2, dtype="uint8")
        got = infer_tile(ensemble, raster, overlap=o, blend="crop", **kw)
        assert got.dtype == np.uint8 and got.shape == (h, w)
        assert np.array_equal(got, voted.cpu().numpy()), o
        assert np.array_equal(got, torch.mode(stack.long(), dim=0)[0].numpy().astype(np.uint8)), o
    # hard vote over TTA-averaged members
    singles = [infer_tile(m, raster, overlap=16, blend="average", tta="flips", **kw) for m in members]
    got = infer_tile(ensemble, raster, overlap=16, blend="average", tta="flips", **kw)
    assert np.array_equal(got, torch.mode(torch.from_numpy(np.stack(singles)).long(), dim=0)[0].numpy().astype(np.uint8))
    with pytest.raises(ValueError):
        infer_tile(ensemble, raster, overlap=16, blend="average", return_probs=True, **kw)

    # soft vote: one accumulator, model-major
    o = 16
    ny, nx, _ = _grid(h, w, d, o)
    dev_r = torch.from_numpy(raster[:3].copy()).to(DEV)
    views = tta_views("flips")
    for tta, vw in ((None, ((0, 0),)), ("flips", views)):
        acc = torch.zeros((2, h, w), dtype=torch.float32, device=DEV)
        for m in members:
            lg = m.run_windows(dev_r, d, o, 0, ny * nx, want="logits", views=vw)
            ops.stitch_accumulate(lg, acc, o, 0, views=vw)
        want_map, want_probs = ops.stitch_finalize(acc, want_probs=True)
        ensemble.vote = "soft"
        try:
            got4, probs4 = infer_tile(ensemble, raster, subtile=d, batch_size=4, device=DEV, overlap=o, blend="average",
                                      tta=tta, return_probs=True)
            got64, probs64 = infer_tile(ensemble, raster, subtile=d, batch_size=64, device=DEV, overlap=o, blend="average",
                                        tta=tta, return_probs=True)
        finally:
            ensemble.vote = "hard"
        assert np.array_equal(got4, want_map.cpu().numpy()) and np.array_equal(probs4, want_probs.cpu().numpy()), tta
        assert np.array_equal(got64, got4) and np.array_equal(probs64, probs4), tta

    # M = 1 with a soft vote is the single-model average path, bit for bit
    solo = PyTorchEnsembleInference(ckpts[0], vote="soft")
    got, probs = infer_tile(solo, raster, overlap=o, blend="average", return_probs=True, **kw)
    base, base_probs = infer_tile(members[0], raster, overlap=o, blend="average", return_probs=True, **kw)
    assert np.array_equal(got, base) and np.array_equal(probs, base_probs)
    with pytest.raises(ValueError):
        PyTorchEnsembleInference(ckpts[0], ckpts[1])
    with pytest.raises(ValueError):
        PyTorchEnsembleInference(ckpts[0], ckpts[1], vote="soft")
    with pytest.raises(ValueError):
        PyTorchEnsembleInference(ckpts[0], vote="mean")
