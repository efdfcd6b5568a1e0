"""The un-rounded mode of the training oracle (oracle/unet_bf16_ref.py, ``rounding=False``) checked against itself on the
CPU — the harness of tests/test_fp32_e2e_gpu.py without the GPU:

* self-closure: a free fp32 run (torch CPU) recorded tensor by tensor and forced into an fp64 instance.  That is what
  the GPU test does with the HIP path's tensors, so the distance measured here is the reference's own share of the
  bounds there (2e-5 of max|ref| per tensor, 1e-4 per BatchNorm coefficient vector, 2e-5 per parameter gradient).
  Bound here 5e-6; measured (16 threads):

      arch    B,H,W,C,K       tensors  worst max|err|/max|ref|   worst coefficient   worst gradient rel-L2
      unet    2,64,96,3,2     367      8.5e-7 (L3B0.gin)         5.0e-7              7.3e-7
      unet    2,128,128,4,3   367      1.15e-6 (L2B0.gin1)       2.3e-7              1.5e-6
      resunet 2,64,96,4,3     372      6.5e-7 (L3B0.gin)         3.7e-7              1.2e-6
      unet++  2,64,96,3,2     479      5.7e-7 (L3B0.yd)          5.0e-7              9.2e-7

  (the factor of about 4 up to the bound is for torch / oneDNN accumulation orders at other thread counts)

* the harness sees wiring faults: a recording run that carries ONE fault (its later units consume the faulty tensor,
  like the units after a wrong kernel do) is forced into a clean fp64 oracle.  Only the tensors of the faulty unit leave
  their bound, by at least 100x; every later unit is recomputed from the forced (faulty) inputs and stays inside.  The
  faults: bn2 of a block takes its conv1's scale/shift; a block output without its residual; a skip gradient joined
  twice; a 16-pixel-wide strip of a decoder gradient left unwritten (zero).
"""
import copy
import functools

import pytest
import torch

from oracle import unet_bf16_ref as R
from oracle.resunet_ref import make_resunet_oracle
from oracle.train_ref import loss_from_logits
from oracle.unet_ref import make_oracle
from oracle.unetpp_ref import make_unetpp_oracle

MAKE = {"unet": make_oracle, "resunet": make_resunet_oracle, "unet++": make_unetpp_oracle}
TENSOR_BOUND, COEFF_BOUND, GRAD_BOUND = 2e-5, 1e-4, 2e-5       # the bounds of the GPU test


def _run(o, img, mask):
    lg = o.forward(img).clone().requires_grad_(True)
    loss, _ = loss_from_logits(lg, mask, ("GDICE", "FOCAL"))
    loss.backward()
    return o.backward(lg.grad)


class _Faulty(R.Bf16TrainOracle):
    """a recording run with one fault: ``fault(name, value, recorded so far)`` -> the tensor the run goes on with"""
    fault = None

    def _t(self, name, val):
        if self.fault is not None:
            val = self.fault(name, val, self.rec)
        return super()._t(name, val)


@functools.lru_cache(maxsize=None)
def _setup(arch, B, H, W, C, K):
    from deadtrees_amd.data.synthetic import synth_batch
    ref = MAKE[arch](C, K, seed=0).train()
    img, mask = synth_batch(B, H, W, C, K, seed=3)
    return ref, img, mask


def _record_and_force(arch, B, H, W, C, K, fault=None):
    """fp32 run with record=True (carrying `fault`) -> the fp64 oracle it was forced into, (fp32, fp64) gradients"""
    ref, img, mask = _setup(arch, B, H, W, C, K)
    a = _Faulty(copy.deepcopy(ref), torch.float32, record=True, update_running=False, rounding=False)
    a.fault = fault
    ga = _run(a, img, mask)
    forced = dict(a.rec)
    forced.update({f"grad:{k}": g for k, g in ga.items()})
    b = R.Bf16TrainOracle(copy.deepcopy(ref), torch.float64, forced=forced, update_running=False, rounding=False)
    gb = _run(b, img, mask)
    return b, ga, gb


def _grad_errs(ga, gb):
    assert set(ga) == set(gb)
    gscale = max(float(g.norm()) for g in gb.values())
    return {k: (float((ga[k].double() - gb[k].double()).norm()), float(gb[k].norm()), gscale) for k in gb}


@pytest.mark.parametrize("arch,B,H,W,C,K,n_min", [("unet", 2, 64, 96, 3, 2, 360), ("unet", 2, 128, 128, 4, 3, 360),
                                                  ("resunet", 2, 64, 96, 4, 3, 360), ("unet++", 2, 64, 96, 3, 2, 360)])
def test_unrounded_oracle_closes_on_its_own_fp32_run(arch, B, H, W, C, K, n_min):
    b, ga, gb = _record_and_force(arch, B, H, W, C, K)
    assert b.unforced == []
    wt = max((v[1], k) for k, v in b.errs.items() if ".bn." not in k)
    wc = max((v[1], k) for k, v in b.errs.items() if ".bn." in k)
    ge = _grad_errs(ga, gb)
    wg = max((e / (n + 1e-30), k) for k, (e, n, _) in ge.items())
    print(f"[fp32 oracle self-closure {arch} {B}x{H}x{W}x{C} K={K}] {len(b.errs)} tensors; worst max-rel {wt[1]} {wt[0]:.2e}; "
          f"worst BatchNorm coefficient {wc[1]} {wc[0]:.2e}; worst parameter gradient {wg[1]} {wg[0]:.2e}")
    assert len(b.errs) >= n_min, len(b.errs)
    for k, (rel, mx) in b.errs.items():
        assert mx <= 5e-6, (k, rel, mx)
    for k, (e, n, gscale) in ge.items():
        assert e <= 5e-6 * n + 1e-6 * gscale, (k, e, n)


def _swap_bn2_coefficients(name, val, rec):
    for c in ("scale", "shift"):
        if name == f"L1B1.y2.bn.{c}":
            return rec[f"L1B1.y1.bn.{c}"].to(val.dtype)
    return val


def _drop_residual(name, val, rec):
    if name == "L2B1.out":
        return torch.relu(R._aff32(rec["L2B1.y2"], rec["L2B1.y2.bn.scale"], rec["L2B1.y2.bn.shift"])).to(val.dtype)
    return val


def _join_skip_twice(name, val, rec):
    if name == "L1B0.gin1":      # layer2.0's input gradient starts from decoder block 2's skip gradient
        return val + rec["D2.dskip"].to(val.dtype)
    return val


def _unwritten_strip(name, val, rec):
    if name == "D4.g":
        val = val.clone()
        val[:, :, :, 16:32] = 0
    return val


@pytest.mark.parametrize("fault,unit", [(_swap_bn2_coefficients, ("L1B1.y2.bn.scale", "L1B1.y2.bn.shift")),
                                        (_drop_residual, ("L2B1.out",)),
                                        (_join_skip_twice, ("L1B0.gin1",)),
                                        (_unwritten_strip, ("D4.g",))])
def test_one_faulty_unit_leaves_the_bound_alone_and_by_100x(fault, unit):
    b, ga, gb = _record_and_force("unet", 2, 64, 96, 3, 2, fault=fault)
    assert b.unforced == []
    bound = lambda k: COEFF_BOUND if ".bn." in k else TENSOR_BOUND      # noqa: E731
    out = {k: mx for k, (_, mx) in b.errs.items() if mx > bound(k)}
    print(f"[fp32 oracle, fault {fault.__name__}] outside the bound: " + ", ".join(f"{k} {v:.2e}" for k, v in out.items()))
    assert set(out) == set(unit), out
    for k, mx in out.items():
        assert mx >= 100 * bound(k), (k, mx)
    # the run that carries the fault is consistent downstream of it: every parameter gradient stays inside
    for k, (e, n, gscale) in _grad_errs(ga, gb).items():
        assert e <= GRAD_BOUND * n + 1e-6 * gscale, (k, e, n)


def test_rounding_is_the_default():
    ref, img, mask = _setup("unet", 2, 64, 96, 3, 2)
    a = R.Bf16TrainOracle(copy.deepcopy(ref), torch.float32, update_running=False)
    b = R.Bf16TrainOracle(copy.deepcopy(ref), torch.float32, update_running=False, rounding=False)
    la, lb = a.forward(img), b.forward(img)
    assert a.rounding and not b.rounding
    rel = float((la - lb).norm() / lb.norm())
    assert 1e-4 < rel < 0.5, rel          # bf16 roundings are there by default and gone un-rounded
