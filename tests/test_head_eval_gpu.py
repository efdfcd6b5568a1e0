"""The fused evaluation head (dt_head_eval / dt_head_eval_bf16 / dt_eval_accumulate, csrc/head_loss.hip).

Integer results — arg-max map, both confusion planes, the accumulator slots 0, 6, 7 — against the unfused device chain
``head_fwd -> loss_sums -> confusion_matrix``: EXACT, because both kernels compute the logits through one device function.
Real-valued results — slots 1-5 and the eight ``parts`` after ``dt_seg_loss_algebra`` — against fp64 on the CPU
(``torch.conv2d`` in fp64 + oracle/losses_ref.py): rel 1e-5 / abs 1e-6, the bound tests/test_loss_kernels_gpu.py puts on
the unfused kernels; the measured error of both paths goes to the parity report.

Inputs: seeded random x / w / bias / labels / dist, lu from {0, 1, 2}.  [p > 0.5] must mean the same in fp32 and fp64,
so a case takes the first seed (from a fixed start) whose fp64 probabilities all stay 1e-4 away from 0.5 — a property of
the reference alone, asserted below.  ``dist`` is drawn from [0, 20): the bound on slot 5 is relative to the SUM, which
only means something while the terms do not cancel (signed maps from the device distance transform run through the same
kernel in tests/test_validate_gpu.py, and the unfused kernel's signed sums are bounded against sum |term| in
tests/test_loss_kernels_gpu.py).  Shapes: one tile (8 x 32), partial tiles, 27 tiles per image (16 + a remainder
chunk of 11 for the 16 tiles a workgroup walks), K = 2, 3, 4, bf16 input, and a call without lu and dist.

Focal gamma: 2.0 everywhere, and 0.0 / 0.5 (the ``gamma == 0`` shortcut and the ``powf`` branch of loss_pixel_sums, which
the fused kernel shares with seg_loss_fwd_kernel) on ``partial`` and ``k4``.  There slot 3 is additionally held to
1e-6 * sum |term| against fp64 ``(1 - p) ** gamma * t * log(p + 1e-10)``, the bound
test_loss_kernels_gpu.py::test_accumulators_probs_and_scratch_layout puts on that slot."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
NACC = 10

#        id              B  K  H   W   bf16   lu/dist  losses
CASES = {"one_tile":     (2, 2, 8, 32, False, True, ("GDICE", "FOCAL", "BOUNDARY")),
         "partial":      (3, 3, 21, 17, False, True, ("DICE", "FOCAL", "BOUNDARY")),
         "remainder":    (2, 2, 72, 96, False, True, ("GDICE", "FOCAL", "BOUNDARY")),
         "k4":           (1, 4, 16, 64, False, True, ("GDICE", "BOUNDARY-RAMPED", "FOCAL")),
         "bf16":         (2, 2, 40, 70, True, True, ("GDICE", "FOCAL", "BOUNDARY")),
         "no_lu_dist":   (2, 3, 21, 17, False, False, ("GDICE", "FOCAL"))}
ALPHA = 0.37
GAMMA_CASES = [(name, 2.0) for name in CASES] + [(name, g) for name in ("partial", "k4") for g in (0.0, 0.5)]


def _inputs(seed, B, K, H, W, bf16):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, H, W, 16), generator=g)
    if bf16:
        x = x.bfloat16()
    w = torch.randn((K, 3, 3, 16), generator=g) * 0.25
    bias = torch.randn(K, generator=g)
    labels = torch.randint(0, K, (B, H, W), generator=g)
    lu = torch.randint(0, 3, (B, H, W), generator=g)
    dist = torch.rand((B, K, H, W), generator=g) * 20
    return x, w, bias, labels, lu, dist


def _logits64(x, w, bias):
    return torch.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), bias.double(), padding=1)


@functools.lru_cache(maxsize=None)
def _case(name, gamma=2.0):
    """inputs + the fp64 reference of a case, computed once and shared (nothing below writes to them)"""
    from test_loss_kernels_gpu import _oracle64
    B, K, H, W, bf16, full, names = CASES[name]
    for seed in range(100 * len(name), 100 * len(name) + 50):
        x, w, bias, labels, lu, dist = _inputs(seed, B, K, H, W, bf16)
        z = _logits64(x, w, bias)
        p = z.softmax(1)
        if float((p - 0.5).abs().min()) >= 1e-4:
            break
    else:
        raise AssertionError("no seed keeps the probabilities off 0.5")
    if not full:
        lu = dist = None
    t = torch.stack([(labels == k) for k in range(K)], 1).double()
    lp = torch.log(p + 1e-10)
    wgt = torch.ones_like(p) if gamma == 0 else (1 - p) ** gamma
    terms = [p * t, p, wgt * t * lp, t * lp, p * dist.double() if dist is not None else torch.zeros_like(p)]
    slots = torch.stack([v.sum(dim=(2, 3)) for v in terms], -1)          # [B,K,5]: slots 1..5
    parts, _ = _oracle64(z, labels, names, dist, ALPHA, gamma)
    return dict(x=x, w=w, bias=bias, labels=labels, lu=lu, dist=dist, K=K, names=names, slots=slots, parts=parts,
                gamma=gamma, focal_mag=terms[2].abs().sum(dim=(2, 3)))


def _dev(t):
    return None if t is None else t.to(DEV)


def _head_fwd(x, w, bias):
    """dt_head_fwd / dt_head_fwd_bf16 -> (logits, int64 arg-max)"""
    from deadtrees_amd import _lib, ops
    if x.dtype != torch.bfloat16:
        return ops.head_fwd(x, w, bias, argmax="int64")
    B, H, W, Cin = x.shape
    K = w.shape[0]
    logits = torch.empty((B, K, H, W), dtype=torch.float32, device=x.device)
    am = torch.empty((B, H, W), dtype=torch.int64, device=x.device)
    _lib.check(_lib.load().dt_head_fwd_bf16(x.data_ptr(), w.data_ptr(), bias.data_ptr(), logits.data_ptr(), am.data_ptr(),
                                            None, B, H, W, Cin, K, _lib.stream()), "dt_head_fwd_bf16")
    return logits, am


def _unfused(c):
    from deadtrees_amd import ops
    from deadtrees_amd.loss.seg_loss import loss_sums
    logits, am = _head_fwd(_dev(c["x"]), _dev(c["w"]), _dev(c["bias"]))
    acc, _, err = loss_sums(logits, _dev(c["labels"]), _dev(c["dist"]), c["gamma"])
    counts, err_cm = ops.confusion_matrix(am, _dev(c["labels"]), _dev(c["lu"]), K=c["K"])
    return acc, am, counts, max(int(err), int(err_cm))


def _fused(c, **kw):
    from deadtrees_amd import ops
    return ops.head_eval(_dev(c["x"]), _dev(c["w"]), _dev(c["bias"]), _dev(c["labels"]), _dev(c["lu"]), _dev(c["dist"]),
                         c["gamma"], want_argmax=True, **kw)


def _parts(acc, c):
    from deadtrees_amd.loss.seg_loss import PART_KEYS, loss_algebra
    B, H, W, _ = c["x"].shape
    parts = loss_algebra(acc, c["names"], B, c["K"], H, W, c["dist"] is not None, ALPHA, c["gamma"])[0]
    assert float(parts[7]) == float(parts[6])
    return {k: float(parts[i]) for i, k in enumerate(PART_KEYS)}


def _rel_err(got, want):
    return float(((got - want).abs() / want.abs().clamp_min(1e-30)).max())


@pytest.mark.parametrize("name,gamma", GAMMA_CASES,
                         ids=[name if g == 2.0 else f"{name}-gamma{g}" for name, g in GAMMA_CASES])
def test_fused_head_against_the_unfused_chain_and_fp64(name, gamma):
    from conftest import parity_report
    c = _case(name, gamma)
    if gamma != 2.0:
        name = f"{name} gamma={gamma}"
    K = c["K"]
    acc, counts, am, err = _fused(c)
    acc_u, am_u, counts_u, err_u = _unfused(c)
    assert int(err) == 0 and err_u == 0
    assert acc.dtype == torch.float64 and tuple(acc.shape) == (c["x"].shape[0], K, NACC)
    # ---- integers: exact
    assert am.dtype == torch.uint8 and torch.equal(am.long(), am_u)
    assert torch.equal(counts, counts_u)
    n = c["labels"].numel()
    assert int(counts[0].sum()) == n
    assert int(counts[1].sum()) == (int((c["lu"] == 1).sum()) if c["lu"] is not None else 0)
    for j in (0, 6, 7):
        assert torch.equal(acc[..., j], acc_u[..., j]), j
    assert float(acc[..., 8:].abs().max()) == 0.0                       # GWDICE slots: zero here
    assert float(acc[..., 0].sum()) == n
    # ---- real-valued slots against fp64
    got, got_u, want = acc[..., 1:6].cpu(), acc_u[..., 1:6].cpu(), c["slots"]
    parity_report(f"[head_eval {name}] slots 1-5 max rel err vs fp64: fused {_rel_err(got, want):.2e}, "
                  f"unfused {_rel_err(got_u, want):.2e}")
    for idx in torch.cartesian_prod(*[torch.arange(s) for s in want.shape]).tolist():
        b, k, j = idx
        assert float(got[b, k, j]) == pytest.approx(float(want[b, k, j]), rel=1e-5, abs=1e-6), (name, b, k, j + 1)
    if gamma != 2.0:
        err3, bound3 = (got[..., 2] - want[..., 2]).abs(), 1e-6 * c["focal_mag"]
        parity_report(f"[head_eval {name}] slot 3 worst |err| / sum|term| vs fp64: "
                      f"{float((err3 / c['focal_mag'].clamp_min(1e-300)).max()):.2e} (bound 1e-6)")
        assert not bool((err3 > bound3).any()), (name, err3.tolist(), bound3.tolist())
    # ---- the eight parts after the algebra
    parts, parts_u = _parts(acc, c), _parts(acc_u, c)
    worst = max(abs(parts[k] - v) / max(abs(v), 1e-30) for k, v in c["parts"].items())
    worst_u = max(abs(parts_u[k] - v) / max(abs(v), 1e-30) for k, v in c["parts"].items())
    parity_report(f"[head_eval {name}] parts max rel err vs fp64: fused {worst:.2e}, unfused {worst_u:.2e}")
    assert set(parts) == set(c["parts"])
    for k, v in c["parts"].items():
        assert parts[k] == pytest.approx(v, rel=1e-5, abs=1e-6), (name, k, parts[k], v)
    assert parts["dice"] == parts_u["dice"] and parts["dice_with_bg"] == parts_u["dice_with_bg"]


def test_counts_accumulate_and_sums_are_overwritten():
    c = _case("remainder")
    acc1, counts, _, err = _fused(c)
    once = counts.clone()
    acc2, counts2, _, _ = _fused(c, counts=counts, err=err)
    assert counts2 is counts and torch.equal(counts, 2 * once)
    assert torch.equal(acc1, acc2) and int(err) == 0                   # fixed-order sums: bit-identical, not doubled


def test_label_equal_to_k_sets_the_flag_and_is_counted_nowhere():
    c = dict(_case("partial"))
    K = c["K"]
    bad = c["labels"].clone()
    bad[1, 3, 5] = K
    bad[2, 20, 16] = -1
    c["labels"] = bad
    acc, counts, am, err = _fused(c)
    torch.cuda.synchronize()
    assert int(err) == 1
    n = bad.numel()
    assert int(counts[0].sum()) == n - 2
    assert bool(torch.isfinite(acc).all()) and float(acc[..., 0].sum()) == n - 2
    clean = _fused(_case("partial"))
    assert torch.equal(am, clean[2])                                     # the prediction does not depend on the labels
    assert torch.equal(acc[..., 7], clean[0][..., 7])


def test_eval_accumulate_forms_the_weighted_sums():
    from deadtrees_amd import ops
    g = torch.Generator().manual_seed(5)
    parts = [torch.rand(8, generator=g) for _ in range(3)]
    weights = [2.0, 2.0, 1.0]
    epoch = torch.zeros(9, dtype=torch.float64, device=DEV)
    want = [0.0] * 9
    for p, w in zip(parts, weights):
        ops.eval_accumulate(p.to(DEV), w, epoch)
        for i in range(8):
            want[i] += w * float(p[i])
        want[8] += w
    assert epoch.cpu().tolist() == want
    with pytest.raises(RuntimeError):
        ops.eval_accumulate(parts[0].to(DEV).double(), 1.0, epoch)
