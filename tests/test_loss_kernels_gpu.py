"""The fused loss / metric kernels (second half of csrc/head_loss.hip) against an fp64 oracle, off the golden grid.

seg_loss_fwd / seg_loss_finalize / seg_loss_algebra / seg_loss_bwd / gwdice_possum / gwdice_posgrad turn the logits into
the scalar that is differentiated; tests/test_model_gpu.py pins them only at whole 1024-pixel multiples, K <= 3,
gamma = 2, alpha = 1 and a unit upstream gradient.  Here: every K the dispatch has, pixel counts around the 256-thread
and 4096-pixel chunk edges, other focal exponents, ramped boundary weights, the accumulators and ``probs`` themselves,
degenerate masks, saturated logits, out-of-range labels, and the integer kernels next to them (confusion matrix,
ensemble vote).  The oracle is oracle/losses_ref.py (fp64, pinned to the imported reference by
tests/test_oracle_golden.py) evaluated on the same fp32 logits.

Tolerances.
  well-conditioned : the bounds of test_fused_losses_vs_reference_golden: values rel 1e-5 / abs 1e-6, gradient
                     rtol 2e-4, atol 2e-6 * max|ref| + 1e-10.
  yardstick        : (degenerate inputs, gamma 3.5, 512 x 512) the rule of test_train_step_gradient_parity: the same
                     oracle runs in fp32 on the CPU; the HIP error against fp64 may be 4x the fp32 oracle's own error
                     (for a gradient: its largest elementwise error) on top of the well-conditioned floor.  The measured
                     ratio goes to the parity report.
  accumulators     : |err| <= 1e-6 * sum |term| per entry (~8 fp32 ulp per pixel term, summed in fp64); where the
                     torch-CPU fp32 pipeline summed in fp64 is itself further off, 4x its error (reported).
  hard thresholds  : no fp64 probability lies within 1e-4 of 0.5 (the generator nudges offending logits, the test
                     asserts it), so [p > 0.5] is the same in fp32 and fp64 and no pixel is excluded anywhere.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
NACC = 10
CHUNK = 4096          # LOSS_PIX_PER_WG of csrc/head_loss.hip
FP32_TINY = 1.1754943508222875e-38

# H*W = 1, 63, 255, 256, 257, 4095, 4096, 4097, 2*4096+1, 5000, 37*53, 131*67: below one wave, around the 256-thread
# block, around one / two / three chunks with a ragged tail
SMALL_SHAPES = [(1, 1), (7, 9), (15, 17), (16, 16), (1, 257), (63, 65), (64, 64), (17, 241), (3, 2731), (1, 5000),
                (37, 53), (131, 67)]
COMBOS = [(("GDICE", "FOCAL"), 1.0), (("DICE", "FOCAL", "BOUNDARY"), 1.0),
          (("GDICE", "BOUNDARY-RAMPED", "FOCAL"), 0.01), (("GDICE", "BOUNDARY-RAMPED", "FOCAL"), 0.37),
          (("GDICE", "BOUNDARY-RAMPED", "FOCAL"), 0.99), (("GWDICE", "FOCAL"), 1.0),
          (("GDICE",), 1.0), (("DICE",), 1.0), (("GWDICE",), 1.0), (("FOCAL",), 1.0), (("BOUNDARY",), 1.0)]
DICE_NAMES = ("GDICE", "DICE", "GWDICE")


# ---------------------------------------------------------------------------------------------- inputs
def _nudge(logits):
    """move every logit vector with an fp64 probability within 1e-4 of 0.5 away from it (deterministic: +0.25 on
    the lowest offending class of the pixel, repeated); returns the nudged fp32 logits"""
    logits = logits.clone()
    for _ in range(8):
        p = logits.double().softmax(1)
        near = (p - 0.5).abs() < 1e-4
        if not bool(near.any()):
            return logits
        first = near.int().argmax(1, keepdim=True)
        logits.scatter_add_(1, first, 0.25 * near.any(1, keepdim=True).float())
    raise AssertionError("could not move the probabilities off 0.5")


def _assert_off_threshold(logits):
    p = logits.double().softmax(1)
    assert float((p - 0.5).abs().min()) >= 1e-4


def _labels(g, B, K, H, W):
    """per-pixel random labels on tiny images, 5 x 5 blobs (cropped) on larger ones; ~55 % background"""
    if H * W < 256:
        fg = torch.rand((B, H, W), generator=g) < 0.45
        return (fg * torch.randint(1, K, (B, H, W), generator=g)).to(torch.int64)
    gh, gw = -(-H // 5), -(-W // 5)
    fg = torch.rand((B, gh, gw), generator=g) < 0.45
    lab = fg * torch.randint(1, K, (B, gh, gw), generator=g)
    return lab.repeat_interleave(5, 1).repeat_interleave(5, 2)[:, :H, :W].contiguous().to(torch.int64)


def _distmap(mask, K):
    from oracle.losses_ref import dist_map, one_hot
    oh = one_hot(mask, K).numpy()
    return torch.from_numpy(np.stack([dist_map(oh[i]) for i in range(oh.shape[0])]).astype(np.float32))


def _case(seed, B, K, H, W, scale=3.0, random_dist=False):
    g = torch.Generator().manual_seed(seed)
    logits = _nudge(torch.randn((B, K, H, W), generator=g) * scale)
    mask = _labels(g, B, K, H, W)
    if random_dist:   # the kernel does not care where the map came from
        dist = (torch.rand((B, K, H, W), generator=g) * 40 - 20).float()
    else:
        dist = _distmap(mask, K)
    return logits, mask, dist


# ---------------------------------------------------------------------------------------------- oracle
def _kind(names):
    k = [n for n in names if n in DICE_NAMES]
    return k[-1] if k else None


def _oracle64(logits, mask, names, dist=None, alpha=1.0, gamma=2.0, gscale=1.0):
    """fp64 oracle on the fp32 logits -> (parts as floats, d(gscale * total)/d logits fp64)"""
    from oracle import losses_ref as L
    K = logits.shape[1]
    lg = logits.double().clone().requires_grad_(True)
    p = lg.softmax(1)
    fg, al = list(range(1, K)), list(range(K))
    kind = _kind(names)
    use_bd = ("BOUNDARY" in names or "BOUNDARY-RAMPED" in names) and dist is not None
    w = alpha if "BOUNDARY-RAMPED" in names else 1.0
    parts = {"dice_loss": 0.0, "boundary_loss": 0.0, "focal_loss": 0.0}
    if kind in ("GDICE", "DICE"):
        total, cp = L.compound_loss(p, mask, names, dist.double() if use_bd else None, alpha, gamma)
        parts.update({k: float(v.detach()) for k, v in cp.items() if k != "total_loss"})
    else:   # GWDICE or a single non-dice term: composed from the same pinned pieces
        total = 0.0
        if kind == "GWDICE":
            d = L.gwdice(p, mask)
            parts["dice_loss"] = float(d.detach())
            total = total + d
        if use_bd:
            b = L.boundary(p, dist.double(), fg)
            parts["boundary_loss"] = float(b.detach())
            total = total + w * b
        if "FOCAL" in names:
            f = L.focal(p, mask, al, gamma)
            parts["focal_loss"] = float(f.detach())
            total = total + f
    parts["ce_loss"] = float(L.cross_entropy(p.detach(), mask, al))
    parts["dice"] = float(L.fscore(p.detach(), mask, ignore_channels=(0,)))
    parts["dice_with_bg"] = float(L.fscore(p.detach(), mask))
    parts["total_loss"] = float(total.detach())
    (gscale * total).backward()
    return parts, lg.grad


def _oracle32(logits, mask, names, dist=None, alpha=1.0, gamma=2.0):
    """the same arithmetic in fp32 on the CPU (oracle/train_ref.py) -> (parts, gradient); the yardstick's other side"""
    from oracle import train_ref as T
    K = logits.shape[1]
    lg = logits.float().clone().requires_grad_(True)
    use_bd = ("BOUNDARY" in names or "BOUNDARY-RAMPED" in names) and dist is not None
    total, p = T.loss_from_logits(lg, mask, names, dist if use_bd else None, alpha, gamma)
    total.backward()
    with torch.no_grad():
        t = T.onehot_f32(mask, K)
        fg, al = list(range(1, K)), list(range(K))
        kind = _kind(names)
        parts = {"dice_loss": 0.0, "boundary_loss": 0.0, "focal_loss": 0.0}
        if kind == "GDICE":
            parts["dice_loss"] = float(T.gdice_t(p, t))
        elif kind == "DICE":
            parts["dice_loss"] = float(T.dice_t(p, t, fg))
        elif kind == "GWDICE":
            from oracle.losses_ref import gwdice
            parts["dice_loss"] = float(gwdice(p, mask))
        if use_bd:
            parts["boundary_loss"] = float(T.boundary_t(p, dist, fg))
        if "FOCAL" in names:
            parts["focal_loss"] = float(T.focal_t(p, t, al, gamma))
        parts["ce_loss"] = float(T.focal_t(p, t, al, 0))
        parts["total_loss"] = float(total.detach())
    return parts, lg.grad


# ---------------------------------------------------------------------------------------------- device side
def _hip(logits, mask, names, dist=None, alpha=1.0, gamma=2.0, gscale=None):
    """-> (parts as floats, d total / d logits on the CPU, err flag).  Compounds with a dice term go through the public
    ``seg_loss`` and autograd; single non-dice terms through ``loss_forward`` / ``loss_backward`` with ``allow_no_dice``
    (what loss/callables.py does)."""
    from deadtrees_amd.loss.seg_loss import PART_KEYS, loss_backward, loss_forward, seg_loss
    lg = logits.to(DEV).requires_grad_(True)
    m = mask.to(DEV)
    d = None if dist is None else dist.to(DEV)
    if _kind(names) is not None:
        total, parts, err = seg_loss(lg, m, d, names, alpha=alpha, gamma=gamma)
        (total if gscale is None else gscale * total).backward()
        grad = lg.grad
        parts = {k: float(v) for k, v in parts.items()}
        assert float(total.detach()) == parts["total_loss"]
    else:
        cfg = {"losses": tuple(names), "alpha": alpha, "gamma": gamma, "allow_no_dice": True}
        pt, err, saved = loss_forward(lg.detach(), m, d, cfg)
        gt = None if gscale is None else torch.tensor(float(gscale), dtype=torch.float32, device=DEV)
        grad = loss_backward(saved, gt)
        parts = {k: float(pt[i]) for i, k in enumerate(PART_KEYS)}
        assert float(pt[7]) == parts["total_loss"]
    return parts, grad.detach().cpu(), int(err)


def _grad_floor(ref):
    return 2e-4 * ref.abs() + 2e-6 * float(ref.abs().max()) + 1e-10


def _check_well_conditioned(got, grad, want, gref, tag=""):
    for k, v in want.items():
        assert got[k] == pytest.approx(v, rel=1e-5, abs=1e-6), (tag, k, got[k], v)
    excess = (grad.double() - gref).abs() - _grad_floor(gref)
    assert float(excess.max()) <= 0.0, (tag, "gradient", float(excess.max()), float(gref.abs().max()))


def _check_yardstick(tag, got, grad, want, gref, want32, g32):
    """HIP error vs fp64 <= 4 x (fp32 CPU oracle's error vs fp64) + the well-conditioned floor; ratios reported"""
    from conftest import parity_report
    assert all(math.isfinite(v) for v in got.values()), (tag, got)
    assert bool(torch.isfinite(grad).all()), tag
    worst, worst_k = 0.0, "none"
    for k, v in want.items():
        e_hip = abs(got[k] - v)
        e_ref = abs(want32[k] - v) if k in want32 else 0.0
        assert e_hip <= 4 * e_ref + 1e-5 * abs(v) + 1e-6, (tag, k, got[k], v, want32.get(k))
        r = e_hip / max(e_ref, 1e-5 * abs(v) + 1e-6)      # error over the larger of fp32-CPU error and floor
        if r > worst:
            worst, worst_k = r, f"{k}: HIP {e_hip:.1e}, fp32-CPU {e_ref:.1e}, of {abs(v):.3g}"
    eh = (grad.double() - gref).abs()
    er = float((g32.double() - gref).abs().max())
    excess = eh - _grad_floor(gref) - 4 * er
    scale = float(gref.abs().max())
    parity_report(f"[loss kernels, {tag}] worst value err / max(fp32-CPU err, floor) {worst:.3f} ({worst_k}); gradient max err "
                  f"HIP {float(eh.max()):.2e} / fp32-CPU {er:.2e} = {float(eh.max()) / er if er > 0 else 0.0:.2f} (max |grad| {scale:.2e})")
    assert float(excess.max()) <= 0.0, (tag, "gradient", float(eh.max()), er, scale)


# ================================================================================================ a. sweep
@pytest.mark.parametrize("B", [1, 2, 5])
@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("H,W", SMALL_SHAPES, ids=[f"{h}x{w}" for h, w in SMALL_SHAPES])
def test_values_and_gradients_over_shapes_classes_and_compounds(H, W, K, B):
    logits, mask, dist = _case(1000 * K + 10 * B + (H * W) % 7, B, K, H, W)
    _assert_off_threshold(logits)
    for names, alpha in COMBOS:
        tag = f"{'+'.join(names)} a={alpha} B={B} K={K} {H}x{W}"
        if "GWDICE" in names and K == 4:   # the reference defines the label-distance matrix for 2 or 3 classes only
            with pytest.raises(NotImplementedError):
                _hip(logits, mask, names, dist, alpha)
            continue
        want, gref = _oracle64(logits, mask, names, dist, alpha)
        got, grad, err = _hip(logits, mask, names, dist, alpha)
        assert err == 0, tag
        assert set(got) == set(want)
        _check_well_conditioned(got, grad, want, gref, tag)


@pytest.mark.parametrize("B,K,names,alpha", [(2, 2, ("GDICE", "FOCAL"), 1.0), (1, 3, ("GWDICE", "FOCAL"), 1.0),
                                             (5, 4, ("DICE", "FOCAL", "BOUNDARY"), 1.0),
                                             (2, 3, ("GDICE", "BOUNDARY-RAMPED", "FOCAL"), 0.37)])
def test_values_and_gradients_at_the_training_tile_size(B, K, names, alpha):
    """512 x 512 (64 chunks per image): seeded random float distance maps; yardstick tolerance"""
    logits, mask, dist = _case(77 + K, B, K, 512, 512, random_dist=True)
    _assert_off_threshold(logits)
    want, gref = _oracle64(logits, mask, names, dist, alpha)
    want32, g32 = _oracle32(logits, mask, names, dist, alpha)
    got, grad, err = _hip(logits, mask, names, dist, alpha)
    assert err == 0
    _check_yardstick(f"{'+'.join(names)} a={alpha} B={B} K={K} 512x512", got, grad, want, gref, want32, g32)


# ================================================================================================ b. accumulators
def _acc_terms(p, mask, dist, gamma, K, with_gw):
    """the ten per-pixel quantities whose per-(sample, class) sums dt_seg_loss_fwd returns, in the dtype of ``p``
    [B,K,H,W] (restated from include/deadtrees_hip.h / the kernel):
      0 t            1 p t          2 p            3 (1-p)^gamma t log(p + 1e-10)     4 t log(p + 1e-10)
      5 p dist       6 t [p > 0.5]  7 [p > 0.5]
      8 t wass,  wass_k = sum_l M[k][l] softmax(p)_l     (GWDICE: a second softmax over the probabilities)
      9 t V,     V(s) = sum over the samples j of (1 - wass of sample j's own label at s)
    with t the one-hot of the label."""
    from oracle.losses_ref import GWDICE_M3
    t = torch.stack([(mask == k) for k in range(K)], 1).to(p.dtype)
    lp = torch.log(p + 1e-10)
    hard = (p > 0.5).to(p.dtype)
    wgt = torch.ones_like(p) if gamma == 0 else (1 - p) ** gamma
    terms = [t, p * t, p, wgt * t * lp, t * lp, p * dist.to(p.dtype), t * hard, hard]
    if with_gw:
        M = torch.tensor(GWDICE_M3, dtype=p.dtype)[:K, :K]
        q = p.softmax(1)
        wass = torch.einsum("kl,blhw->bkhw", M, q)
        V = (1 - (t * wass).sum(1)).sum(0)                 # [H,W]
        terms += [t * wass, t * V[None, None]]
    else:
        terms += [torch.zeros_like(p), torch.zeros_like(p)]
    return torch.stack(terms, -1)                          # [B,K,H,W,10]


ACC_CASES = [(1, 2, 1, 1), (2, 3, 7, 9), (5, 4, 15, 17), (2, 2, 16, 16), (1, 3, 1, 257), (2, 4, 63, 65), (5, 2, 64, 64),
             (2, 3, 17, 241), (1, 4, 3, 2731), (2, 2, 1, 5000), (2, 4, 37, 53), (5, 3, 131, 67), (2, 3, 512, 512)]


@pytest.mark.parametrize("B,K,H,W", ACC_CASES, ids=[f"b{b}k{k}_{h}x{w}" for b, k, h, w in ACC_CASES])
@pytest.mark.parametrize("gamma", [2.0, 0.5])
def test_accumulators_probs_and_scratch_layout(B, K, H, W, gamma):
    from conftest import parity_report
    from deadtrees_amd import _lib
    from deadtrees_amd.loss.seg_loss import gwdice_matrix, loss_sums
    logits, mask, dist = _case(31 * B + K + H, B, K, H, W, scale=3.0 if gamma >= 1 else 1.5, random_dist=H * W > 20000)
    _assert_off_threshold(logits)
    with_gw = K <= 3
    wass_m = gwdice_matrix(K, DEV) if with_gw else None
    acc, probs, err = loss_sums(logits.to(DEV), mask.to(DEV), dist.to(DEV), gamma, want_probs=True, wass_m=wass_m)
    assert int(err) == 0 and tuple(acc.shape) == (B, K, NACC) and acc.dtype == torch.float64
    # --- sizing: [B][K][10] results, then one [K][10] partial row per 4096-pixel chunk and sample
    wpi = -(-H * W // CHUNK)
    n = _lib.load().dt_seg_loss_acc_doubles(B, K, H, W)
    assert n == B * (1 + wpi) * K * NACC
    assert acc.untyped_storage().nbytes() == 8 * n and acc.storage_offset() == 0
    # --- the partial rows behind the result, read through the storage of the returned view: their fixed-order sum
    # over the chunks IS the result, bit for bit (seg_loss_finalize_kernel)
    whole = torch.empty(0, dtype=torch.float64, device=DEV).set_(acc.untyped_storage())
    assert whole.numel() == n
    part = whole[B * K * NACC:].view(B, wpi, K, NACC).cpu()
    s = torch.zeros((B, K, NACC), dtype=torch.float64)
    for c in range(wpi):
        s = s + part[:, c]
    assert torch.equal(s, acc.cpu())
    # --- values
    p64 = logits.double().softmax(1)
    t64 = _acc_terms(p64, mask, dist, gamma, K, with_gw)
    want = t64.sum(dim=(2, 3))
    mag = t64.abs().sum(dim=(2, 3))
    t32 = _acc_terms(logits.softmax(1), mask, dist, gamma, K, with_gw)
    err32 = (t32.double().sum(dim=(2, 3)) - want).abs()
    bound = 1e-6 * mag
    loose = err32 > bound
    if bool(loose.any()):
        parity_report(f"[loss accumulators b{B}k{K} {H}x{W} gamma={gamma}] torch-CPU fp32 terms summed in fp64 exceed "
                      f"1e-6 * sum|term| at {loose.nonzero().tolist()} (worst {float((err32 / mag.clamp_min(1e-300))[loose].max()):.2e}); "
                      f"bound there 4x that error")
    bound = torch.where(loose, 4 * err32, bound)
    got = acc.cpu()
    for j in (0, 6, 7):   # integer counts
        assert torch.equal(got[..., j], want[..., j]), j
    bad = (got - want).abs() > bound
    assert not bool(bad.any()), (bad.nonzero().tolist(), got[bad].tolist(), want[bad].tolist(), bound[bad].tolist())
    # --- probs: expf of an fp32 difference d = z - max carries |d| * 2^-24 relative error from rounding d alone, plus
    # ~1 ulp each for expf, the K-term sum, the reciprocal and the product: (8 + |d|) * 2^-23 relative, one denormal abs
    d = logits.double().amax(1, keepdim=True) - logits.double()
    tol = p64 * (8 + d) * 2.0 ** -23 + 2 * FP32_TINY
    assert probs.dtype == torch.float32 and tuple(probs.shape) == (B, K, H, W)
    assert not bool(((probs.cpu().double() - p64).abs() > tol).any())


# ================================================================================================ c. focal gamma
@pytest.mark.parametrize("K", [2, 4])
@pytest.mark.parametrize("gamma", [0.0, 0.5, 1.0, 2.0, 3.5])
def test_focal_gamma_values_and_gradients(gamma, K):
    """the powf branches of forward and backward (and gamma == 0 / == 2 shortcuts) through seg_loss(gamma=) and through
    the deadtrees.loss FocalLoss / CrossEntropy callables.  For gamma < 1 the reference's own derivative
    gamma (1-p)^(gamma-1) log p is unbounded as the correct class saturates, so those cases use logits of scale 1.5
    and assert that no probability reaches 1 - 1e-6."""
    from deadtrees.loss.losses import CrossEntropy, FocalLoss
    B, H, W = 2, 37, 53
    logits, mask, _ = _case(5 + K, B, K, H, W, scale=3.0 if gamma >= 1 else 1.5)
    if gamma < 1:
        assert float(logits.double().softmax(1).max()) < 1 - 1e-6
    for names in (("GDICE", "FOCAL"), ("FOCAL",)):
        tag = f"{'+'.join(names)} gamma={gamma} K={K}"
        want, gref = _oracle64(logits, mask, names, None, 1.0, gamma)
        got, grad, err = _hip(logits, mask, names, None, 1.0, gamma)
        assert err == 0
        if gamma > 2:
            want32, g32 = _oracle32(logits, mask, names, None, 1.0, gamma)
            _check_yardstick(tag, got, grad, want, gref, want32, g32)
        else:
            _check_well_conditioned(got, grad, want, gref, tag)
    # the callables take probabilities
    fn = CrossEntropy(idc=list(range(K))) if gamma == 0 else FocalLoss(idc=list(range(K)), gamma=gamma)
    lg = logits.to(DEV).requires_grad_(True)
    val = fn(lg.softmax(1), mask.to(DEV))
    val.backward()
    want, gref = _oracle64(logits, mask, ("FOCAL",), None, 1.0, gamma)
    got = {"focal_loss": float(val.detach())}
    want = {"focal_loss": want["focal_loss"]}
    if gamma > 2:
        want32, g32 = _oracle32(logits, mask, ("FOCAL",), None, 1.0, gamma)
        _check_yardstick(f"FocalLoss callable gamma={gamma} K={K}", got, lg.grad.cpu(), want, gref, want32, g32)
    else:
        _check_well_conditioned(got, lg.grad.cpu(), want, gref, f"callable gamma={gamma}")


# ================================================================================================ d. upstream gradient
@pytest.mark.parametrize("names,K", [(("GDICE", "FOCAL"), 4), (("DICE", "FOCAL", "BOUNDARY"), 3), (("GWDICE", "FOCAL"), 3),
                                     (("FOCAL",), 2)])
def test_upstream_gradient_scale(names, K):
    """the kernel applies the upstream gradient as one final multiply: a power of two scales every normal-number entry
    exactly; 0.3 is compared against the oracle's gradient of 0.3 * loss"""
    B, H, W = 2, 37, 53
    logits, mask, dist = _case(11 + K, B, K, H, W)
    _, g1, _ = _hip(logits, mask, names, dist)
    for s in (2.0 ** -6, 2.0 ** 10):
        _, gs, _ = _hip(logits, mask, names, dist, gscale=s)
        want = g1 * s
        normal = (g1.abs() >= FP32_TINY) & (want.abs() >= FP32_TINY) & torch.isfinite(want)
        assert float(normal.float().mean()) > 0.9
        assert torch.equal(gs[normal], want[normal]), s
    _, g03, _ = _hip(logits, mask, names, dist, gscale=0.3)
    _, gref = _oracle64(logits, mask, names, dist, gscale=0.3)
    _check_well_conditioned({}, g03, {}, gref, f"{names} gscale=0.3")
    assert float((g03 - g1).abs().max()) > 0     # the scale arrived


# ================================================================================================ e. degenerate inputs
def _degenerate(kind, K):
    B, H, W = 2, 37, 53
    g = torch.Generator().manual_seed(40 + K)
    logits = torch.randn((B, K, H, W), generator=g) * 3
    mask = _labels(g, B, K, H, W)
    if kind.startswith("absent"):
        k = int(kind[-1])
        mask[mask == k] = (k + 1) % K
        assert not bool((mask == k).any()) and len(mask.unique()) == K - 1
    elif kind == "one_sample_background":
        mask[1] = 0
    elif kind == "all_background":
        mask[:] = 0
    elif kind == "single_foreground_pixel":
        mask[:] = 0
        mask[1, 20, 31] = K - 1
    elif kind == "saturated":
        logits = logits * 40        # fp32 softmax: exact 0 and 1
        p32 = logits.softmax(1)
        assert bool((p32 == 0).any()) and bool((p32 == 1).any())
    elif kind == "equal_logits":
        logits = torch.full((B, K, H, W), 0.75)
    else:
        raise KeyError(kind)
    return _nudge(logits), mask, _distmap(mask, K)


DEGENERATE = ["absent0", "absent1", "absent2", "one_sample_background", "all_background", "single_foreground_pixel",
              "saturated", "equal_logits"]
DEG_COMBOS = [("GDICE", "FOCAL"), ("DICE", "FOCAL", "BOUNDARY"), ("GWDICE", "FOCAL"), ("FOCAL",)]


DEG_PARAMS = [(kind, K) for K in (3, 4) for kind in DEGENERATE] + [("absent3", 4)]


@pytest.mark.parametrize("kind,K", DEG_PARAMS, ids=[f"{kind}-k{K}" for kind, K in DEG_PARAMS])
def test_degenerate_masks_and_logits(kind, K):
    """GDICE weight 1 / (0 + 1e-9) of an absent class, DICE's U -> eps, GWDICE's gtp = 0, log(0 + 1e-10) and
    -(1-p)^2 / (p + 1e-10) at an underflowed softmax, p = 1/K everywhere: finite and as close to fp64 as the yardstick
    allows.  ``equal_logits`` runs at K = 3 and 4 only: at K = 2 every probability would be exactly 0.5, which the
    threshold rule of this file forbids (the nudge would undo the case)."""
    logits, mask, dist = _degenerate(kind, K)
    _assert_off_threshold(logits)
    for names in DEG_COMBOS:
        if "GWDICE" in names and K == 4:
            continue
        tag = f"{kind} {'+'.join(names)} K={K}"
        want, gref = _oracle64(logits, mask, names, dist)
        want32, g32 = _oracle32(logits, mask, names, dist)
        got, grad, err = _hip(logits, mask, names, dist)
        assert err == 0
        _check_yardstick(tag, got, grad, want, gref, want32, g32)


# ================================================================================================ f. labels
def _oracle64_onehot(logits, t, names, gamma=2.0):
    """the fp64 oracle written on an explicit one-hot ``t`` [B,K,H,W] (so that a row of it can be zeroed, which is what
    a label outside [0, K) amounts to in kernels that form t_k = [label == k]).  Formulas of oracle/losses_ref.py:
    gdice / dice / focal verbatim with ``t`` in place of one_hot(mask); gwdice with wass = sum_k t_k (M q)_k and
    alpha(s) = sum_k>0 t_k."""
    from oracle.losses_ref import EPS, GWDICE_M3
    B, K = logits.shape[:2]
    lg = logits.double().clone().requires_grad_(True)
    p = lg.softmax(1)
    kind = _kind(names)
    total = 0.0
    if kind == "GDICE":
        cnt = t.sum(dim=(0, 2, 3))
        w = 1.0 / (cnt * cnt + 1e-9)
        num = (w * (t * p).sum(dim=(0, 2, 3))).sum()
        den = (w * (t + p).sum(dim=(0, 2, 3))).sum()
        total = total + 1.0 - 2.0 * (num + 1e-9) / (den + 1e-9)
    elif kind == "DICE":
        inter = (p * t)[:, 1:].sum(dim=(2, 3))
        union = p[:, 1:].sum(dim=(2, 3)) + t[:, 1:].sum(dim=(2, 3))
        total = total + (1.0 - (2.0 * inter + EPS) / (union + EPS)).mean()
    elif kind == "GWDICE":
        eps = float(np.spacing(1))
        M = torch.tensor(GWDICE_M3, dtype=torch.float64)[:K, :K]
        wass = (t * torch.einsum("kl,blhw->bkhw", M, p.softmax(1))).sum(1)       # [B,H,W]
        alpha = t[:, 1:].sum(1)
        tp = (alpha * (1.0 - wass).sum(0, keepdim=True)).sum(dim=(1, 2))
        all_err = wass.sum(dim=(1, 2))
        total = total + (1.0 - (2.0 * tp + eps) / (2.0 * tp + all_err + eps)).mean()
    if "FOCAL" in names:
        total = total - ((1.0 - p) ** gamma * t * torch.log(p + EPS)).sum() / (t.sum() + EPS)
    total.backward()
    return float(total.detach()), lg.grad


@pytest.mark.parametrize("names", [("GDICE", "FOCAL"), ("DICE", "FOCAL"), ("GWDICE", "FOCAL"), ("FOCAL",)],
                         ids=["GDICE", "DICE", "GWDICE", "NONE"])
@pytest.mark.parametrize("bad_label", [-1, "K"])
def test_out_of_range_label_is_flagged_and_contributes_nothing(names, bad_label):
    """a label of -1 or K at ONE pixel of one sample: the flag is set, everything stays finite, the total equals the
    oracle's with that pixel's one-hot row zeroed, and so does the gradient at every other pixel - the same position in
    the OTHER samples included, which GWDICE's cross-sample position sums (gwdice_possum / gwdice_posgrad, with label
    guards of their own) couple to the bad pixel."""
    B, K, H, W = 3, 3, 37, 53
    logits, mask, _ = _case(91, B, K, H, W)
    y, x = 11, 29
    mask[:, y, x] = torch.tensor([1, 2, 0])       # foreground at the same position of sample 0, whatever the seed gave
    t = torch.stack([(mask == k) for k in range(K)], 1).double()
    # the one-hot oracle is the pinned oracle on clean labels
    clean, gclean = _oracle64_onehot(logits, t, names)
    want, gref = _oracle64(logits, mask, names)
    assert clean == pytest.approx(want["total_loss"], rel=1e-12)
    assert float((gclean - gref).abs().max()) <= 1e-12 * float(gref.abs().max())
    bad = mask.clone()
    bad[1, y, x] = K if bad_label == "K" else -1
    t[1, :, y, x] = 0
    want_total, gref = _oracle64_onehot(logits, t, names)
    got, grad, err = _hip(logits, bad, names)
    assert err == 1
    assert all(math.isfinite(v) for v in got.values()) and bool(torch.isfinite(grad).all())
    assert got["total_loss"] == pytest.approx(want_total, rel=1e-5, abs=1e-6)
    other = torch.ones((B, K, H, W), dtype=torch.bool)
    other[1, :, y, x] = False
    excess = ((grad.double() - gref).abs() - _grad_floor(gref))[other]
    assert float(excess.max()) <= 0.0, (float(excess.max()), float(gref.abs().max()))
    # and the clean labels do not raise the flag
    assert _hip(logits, mask, names)[2] == 0


@pytest.mark.parametrize("dtype", [torch.int32, torch.uint8])
def test_label_dtypes_give_the_int64_result(dtype):
    from deadtrees_amd.loss.seg_loss import seg_loss
    logits, mask, dist = _case(3, 2, 3, 37, 53)
    outs = []
    for m in (mask, mask.to(dtype)):
        lg = logits.to(DEV).requires_grad_(True)
        total, parts, err = seg_loss(lg, m.to(DEV), dist.to(DEV), ("GWDICE", "BOUNDARY", "FOCAL"))
        total.backward()
        outs.append((total.detach().cpu(), torch.stack([parts[k] for k in sorted(parts)]).cpu(), lg.grad.cpu(), int(err)))
    assert outs[0][3] == outs[1][3] == 0
    for a, b in zip(outs[0][:3], outs[1][:3]):
        assert torch.equal(a, b)


# ================================================================================================ g. structure
@pytest.mark.parametrize("names", [("GDICE", "BOUNDARY", "FOCAL"), ("GWDICE", "FOCAL")])
def test_two_identical_calls_are_bit_identical(names):
    """fixed-order reductions, no float atomics: values and gradients repeat exactly (three chunks, ragged tail)"""
    from deadtrees_amd.loss.seg_loss import seg_loss
    logits, mask, dist = _case(8, 5, 3, 131, 67)
    outs = []
    for _ in range(2):
        lg = logits.to(DEV).requires_grad_(True)
        total, parts, _ = seg_loss(lg, mask.to(DEV), dist.to(DEV), names, gamma=3.5)
        total.backward()
        outs.append((torch.stack([parts[k] for k in sorted(parts)]).cpu(), lg.grad.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_accumulator_rows_follow_a_batch_permutation_bit_for_bit():
    """rows 0..8 of acc[b] depend on sample b alone, so permuting the batch permutes them exactly; row 9 (GWDICE) holds
    V, a sum over the batch in batch order, and follows to rounding only"""
    from deadtrees_amd.loss.seg_loss import gwdice_matrix, loss_sums
    B, K, H, W = 5, 3, 131, 67
    logits, mask, dist = _case(9, B, K, H, W)
    perm = torch.tensor([3, 0, 4, 2, 1])
    for wass_m in (None, gwdice_matrix(K, DEV)):
        a, _, _ = loss_sums(logits.to(DEV), mask.to(DEV), dist.to(DEV), 2.0, wass_m=wass_m)
        b, _, _ = loss_sums(logits[perm].to(DEV), mask[perm].to(DEV), dist[perm].to(DEV), 2.0, wass_m=wass_m)
        a, b = a.cpu(), b.cpu()
        last = NACC if wass_m is None else 9
        assert torch.equal(a[perm][..., :last], b[..., :last])
        assert bool((a[..., :9].abs().sum(-1) > 0).all())
        if wass_m is not None:
            assert float(a[..., 9].abs().max()) > 0
            np.testing.assert_allclose(b[..., 9].numpy(), a[perm][..., 9].numpy(), rtol=1e-6)


@pytest.mark.parametrize("K,H,W", [(2, 37, 53), (3, 131, 67), (3, 1, 1)])
def test_gwdice_single_sample_is_the_published_formula(K, H, W):
    """B = 1: the reference's [B,1,S] x [B,S] broadcast collapses and the loss is the published generalised Wasserstein
    Dice,  1 - (2 TP + eps) / (2 TP + sum_s wass(s) + eps),  TP = sum_s [t_s > 0] (1 - wass(s)),
    wass(s) = sum_l M[t_s][l] q_l(s),  q = softmax(softmax(logits))  - written out here, no cross-sample sum."""
    from oracle.losses_ref import GWDICE_M3
    logits, mask, _ = _case(17 + K, 1, K, H, W)
    lg = logits.double().clone().requires_grad_(True)
    q = lg.softmax(1).softmax(1)[0].reshape(K, -1)                       # [K,S]
    t = mask.reshape(-1)
    M = torch.tensor(GWDICE_M3, dtype=torch.float64)[:K, :K]
    wass = (M[t].T * q).sum(0)
    tp = ((t > 0).double() * (1.0 - wass)).sum()
    eps = float(np.spacing(1))
    loss = 1.0 - (2.0 * tp + eps) / (2.0 * tp + wass.sum() + eps)
    loss.backward()
    got, grad, err = _hip(logits, mask, ("GWDICE",))
    assert err == 0
    _check_well_conditioned({"dice_loss": got["dice_loss"], "total_loss": got["total_loss"]}, grad,
                            {"dice_loss": float(loss.detach()), "total_loss": float(loss.detach())}, lg.grad, f"GWDICE B=1 K={K}")


# ================================================================================================ h. callables
def _callable_cases(K):
    from deadtrees.loss.gdl import GeneralizedDiceLoss
    from deadtrees.loss.gwdl import GeneralizedWassersteinDiceLoss
    from deadtrees.loss.losses import BoundaryLoss, CrossEntropy, DiceLoss, FocalLoss, SurfaceLoss
    from oracle.losses_ref import GWDICE_M3
    fg, al = list(range(1, K)), list(range(K))
    cases = [("GeneralizedDiceLoss", GeneralizedDiceLoss(), ("GDICE",), "dice_loss", "onehot"),
             ("DiceLoss", DiceLoss(idc=fg), ("DICE",), "dice_loss", "onehot"),
             ("FocalLoss", FocalLoss(idc=al, gamma=2), ("FOCAL",), "focal_loss", "onehot"),
             ("CrossEntropy", CrossEntropy(idc=al), ("FOCAL",), "ce_loss", "onehot"),
             ("SurfaceLoss", SurfaceLoss(idc=fg), ("BOUNDARY",), "boundary_loss", "dist"),
             ("BoundaryLoss", BoundaryLoss(idc=fg), ("BOUNDARY",), "boundary_loss", "dist")]
    if K <= 3:
        gw = GeneralizedWassersteinDiceLoss(dist_matrix=np.array(GWDICE_M3)[:K, :K])
        cases.append(("GeneralizedWassersteinDiceLoss", gw, ("GWDICE",), "dice_loss", "labels"))
    return cases


@pytest.mark.parametrize("B,K,H,W", [(2, 3, 37, 53), (1, 4, 17, 241), (5, 2, 3, 2731)])
def test_loss_callables_values_and_logit_gradients(B, K, H, W):
    """every deadtrees.loss callable on probs = softmax(leaf logits), off the golden grid: value and d/d logits"""
    from deadtrees.loss.losses import class2one_hot
    logits, mask, dist = _case(23 + K, B, K, H, W)
    for name, fn, names, key, second in _callable_cases(K):
        gamma = 0.0 if name == "CrossEntropy" else 2.0
        want, gref = _oracle64(logits, mask, names, dist, 1.0, gamma)
        lg = logits.to(DEV).requires_grad_(True)
        arg = {"onehot": lambda: class2one_hot(mask.to(DEV), K), "dist": lambda: dist.to(DEV),
               "labels": lambda: mask.to(DEV)}[second]()
        val = fn(lg.softmax(1), arg)
        val.backward()
        ref_val = want["focal_loss"] if name == "CrossEntropy" else want[key]
        _check_well_conditioned({key: float(val.detach())}, lg.grad.cpu(), {key: ref_val}, gref, f"{name} b{B}k{K} {H}x{W}")


def test_callables_gradient_with_respect_to_leaf_probabilities():
    """What loss/callables._fused does: it hands log(probs) to the fused kernel, whose own softmax turns it back into
    probs / sum(probs).  So (1) inputs that do not sum to one are renormalised, and (2) the gradient with respect to a
    LEAF ``probs`` is the reference's gradient g projected onto the simplex' tangent at each pixel,
    g_k - sum_j p_j g_j: the reference's gradient minus its p-weighted mean.  The subtracted term is constant over the
    classes of a pixel, and the softmax Jacobian maps such a term to zero, so d/d logits (the previous test) is the
    reference's; the module docstring of loss/callables.py says exactly this."""
    from deadtrees.loss.losses import FocalLoss, class2one_hot
    from oracle import losses_ref as L
    B, K, H, W = 2, 3, 37, 53
    logits, mask, _ = _case(29, B, K, H, W, scale=1.0)    # moderate logits: d focal / d p ~ 1 / p stays of one scale
    fn = FocalLoss(idc=list(range(K)), gamma=2)
    probs = logits.softmax(1).to(DEV).requires_grad_(True)
    val = fn(probs, class2one_hot(mask.to(DEV), K))
    val.backward()
    p64 = probs.detach().cpu().double().requires_grad_(True)
    ref = L.focal(p64, mask, list(range(K)), 2.0)
    ref.backward()
    g = p64.grad
    pn = p64.detach() / p64.detach().sum(1, keepdim=True)
    projected = g - (pn * g).sum(1, keepdim=True)
    assert float(val.detach()) == pytest.approx(float(ref.detach()), rel=1e-5, abs=1e-6)
    got = probs.grad.cpu().double()
    excess = (got - projected).abs() - _grad_floor(projected)
    assert float(excess.max()) <= 0.0, float(excess.max())
    # ... which is NOT the unprojected reference gradient: that one is exactly zero off the labelled class, the
    # delivered one carries minus the p-weighted mean there
    off = g == 0
    assert bool(off.any()) and float(got[off].abs().max()) > 0.1 * float((pn * g).sum(1).abs().max()) > 0
    # per pixel the delivered gradient is orthogonal to p
    assert float((pn * got).sum(1).abs().max()) <= 1e-5 * float(got.abs().max())
    # unnormalised input: renormalised, the value is that of probs
    val2 = fn(2.0 * probs.detach(), class2one_hot(mask.to(DEV), K))
    assert float(val2) == pytest.approx(float(val.detach()), rel=1e-5, abs=1e-6)


# ================================================================================================ 3. integer kernels
def _confusion_ref(pred, tgt, lu, K):
    ok = (pred >= 0) & (pred < K) & (tgt >= 0) & (tgt < K)
    idx = (tgt[ok] * K + pred[ok]).long()
    all_ = torch.bincount(idx, minlength=K * K).view(K, K)
    masked = torch.bincount(idx[lu[ok] == 1], minlength=K * K).view(K, K)
    return torch.stack([all_, masked]), int(ok.sum())


@pytest.mark.parametrize("K", [2, 4])
@pytest.mark.parametrize("n", [1, 255, 4097, 2048 * 4096 + 4097])
def test_confusion_matrix_sizes_and_classes(K, n):
    """exact counts; above 2048 * 4096 pixels the grid is capped and every thread loops"""
    from deadtrees_amd import ops
    g = torch.Generator().manual_seed(n % 1000 + K)
    pred = torch.randint(0, K, (n,), generator=g)
    tgt = torch.randint(0, K, (n,), generator=g)
    lu = torch.randint(0, 3, (n,), generator=g)
    want, valid = _confusion_ref(pred, tgt, lu, K)
    counts, err = ops.confusion_matrix(pred.to(DEV), tgt.to(DEV), lu.to(DEV), K=K)
    assert int(err) == 0 and valid == n
    assert torch.equal(counts.cpu(), want) and int(counts[0].sum()) == n
    # accumulation across calls into the same counts, uint8 predictions, no land-use mask
    counts, err = ops.confusion_matrix(pred.to(torch.uint8).to(DEV), tgt.to(DEV), None, K=K, counts=counts)
    assert int(err) == 0
    assert torch.equal(counts[0].cpu(), 2 * want[0]) and torch.equal(counts[1].cpu(), want[1])


@pytest.mark.parametrize("K", [2, 4])
def test_confusion_matrix_skips_and_flags_out_of_range_pixels(K):
    from deadtrees_amd import ops
    n = 4097
    g = torch.Generator().manual_seed(K)
    pred = torch.randint(0, K, (n,), generator=g)
    tgt = torch.randint(0, K, (n,), generator=g)
    lu = torch.ones(n, dtype=torch.int64)
    pred[5], pred[4096] = K, -1
    tgt[77], tgt[300] = -1, K + 3
    pred[900], tgt[900] = K, K
    want, valid = _confusion_ref(pred, tgt, lu, K)
    assert valid == n - 5
    counts, err = ops.confusion_matrix(pred.to(DEV), tgt.to(DEV), lu.to(DEV), K=K)
    assert int(err) == 1
    assert torch.equal(counts.cpu(), want)
    assert int(counts[0].sum()) == n - 5 and int(counts[1].sum()) == n - 5      # counted nowhere
    # a clean second call adds to the counts and reports no error of its own
    pred2, tgt2 = pred.clamp(0, K - 1), tgt.clamp(0, K - 1)
    want2, _ = _confusion_ref(pred2, tgt2, lu, K)
    counts, err = ops.confusion_matrix(pred2.to(DEV), tgt2.to(DEV), lu.to(DEV), K=K, counts=counts)
    assert int(err) == 0 and torch.equal(counts.cpu(), want + want2)


def _vote_ref(maps, K):
    """per-pixel most frequent class, ties to the smallest class (numpy argmax returns the first maximum)"""
    cnt = np.stack([(maps.numpy() == k).sum(0) for k in range(K)], 0)
    return torch.from_numpy(cnt.argmax(0))


@pytest.mark.parametrize("M,K,shape", [(1, 8, (4,)), (4, 8, (2, 36, 52)), (6, 2, (1, 4)), (2, 3, (5, 8)), (7, 8, (3, 4100))])
def test_ensemble_vote_up_to_eight_classes_with_ties(M, K, shape):
    from deadtrees_amd import ops
    g = torch.Generator().manual_seed(M * 10 + K)
    maps = torch.randint(0, K, (M,) + shape, generator=g, dtype=torch.uint8)
    if M % 2 == 0:   # an even number of models: plant exact ties; they go to the smaller class
        flat = maps.view(M, -1)
        flat[:M // 2, 0], flat[M // 2:, 0] = K - 1, 0
        flat[:M // 2, 1], flat[M // 2:, 1] = 1, K - 1
    want = _vote_ref(maps, K)
    if M % 2 == 0:
        assert int(want.view(-1)[0]) == 0 and int(want.view(-1)[1]) == 1
    got, err = ops.ensemble_vote(maps.to(DEV), K, dtype="int64")
    assert int(err) == 0 and got.dtype == torch.int64 and torch.equal(got.cpu(), want)
    got8, err = ops.ensemble_vote(maps.to(DEV), K, dtype="uint8")
    assert int(err) == 0 and got8.dtype == torch.uint8 and torch.equal(got8.cpu().long(), want)
    if M == 1:
        assert torch.equal(got8.cpu(), maps[0])


def test_ensemble_vote_rejects_a_pixel_count_off_the_dword_grid():
    """four uint8 pixels per lane: n must be a multiple of 4, and the call says so instead of reading past the maps"""
    from deadtrees_amd import ops
    maps = torch.zeros((3, 6), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.ensemble_vote(maps, 2)
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.ensemble_vote(torch.zeros((3, 8), dtype=torch.uint8, device=DEV), 9)
