"""Both precisions on ONE engine object, alternating: fp32 - bf16 - fp32 and bf16 - fp32 - bf16 training passes (forward +
backward, no optimiser step) of one ``UNetHIP`` per decoder kind.  The two reverse passes share one driver, one
``launches`` record, one set of workspaces (``bn_red*``, ``wgrad_ws``, ``chsum_ws``, the constant vectors) and one side
stream; whatever the pass of the other precision leaves behind in them must not reach the next pass.

The third pass repeats the first on the same weights and input (batch-statistics BatchNorm: the running statistics the
passes in between moved do not enter), so its gradient buffer has to agree with the first's, per parameter tensor, to
twice the bound a single correct step is held to against its oracle — tests/test_fp32_e2e_gpu.py: 2e-5 per gradient,
tests/test_bf16_e2e_gpu.py: 5e-5 — of the tensor's largest element, and ``engine.launches`` has to be the same list.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUND = {"fp32": 2 * 2e-5, "bf16": 2 * 5e-5}


def _pass(m, img, mask, precision):
    """one training-mode forward + backward in `precision` -> (gradients by parameter name, copy of engine.launches)"""
    from deadtrees_amd.loss.seg_loss import seg_loss
    m.precision = precision
    logits = m(img)
    loss, _, err = seg_loss(logits, mask, None, ("GDICE", "FOCAL"))
    loss.backward()
    torch.cuda.synchronize()
    assert int(err) == 0
    return m.smp_grad_dict(), {k: list(v) for k, v in m.engine.launches.items()}


@pytest.mark.parametrize("order", [("fp32", "bf16", "fp32"), ("bf16", "fp32", "bf16")], ids=lambda o: "-".join(o))
@pytest.mark.parametrize("kind", ["unet", "resunet", "unetplusplus"])
def test_third_pass_repeats_the_first_after_a_pass_of_the_other_precision(kind, order):
    from deadtrees_amd.data.synthetic import synth_batch
    from deadtrees_amd.network.unet import UNetHIP
    m = UNetHIP(in_channels=3, classes=2, decoder=kind)
    m.reset_parameters(seed=0)
    m.to(DEV).train()
    eng = m.engine
    img, mask = synth_batch(2, 64, 64, 3, 2, seed=4321)
    img, mask = img.to(DEV), mask.to(DEV)
    (g1, l1), (g2, l2), (g3, l3) = (_pass(m, img, mask, p) for p in order)
    assert m.engine is eng
    worst = max((float((g3[k] - g1[k]).abs().max()) / (float(g1[k].abs().max()) + 1e-30), k) for k in g1)
    print(f"[alternating {kind} {'-'.join(order)}] {len(g1)} parameter tensors, worst max|g3 - g1| / max|g1|: "
          f"{worst[1]} {worst[0]:.2e} (bound {BOUND[order[0]]:.0e}); launches {len(l1['dgrad'])} dgrad / "
          f"{len(l1['wgrad'])} wgrad (first), {len(l2['dgrad'])} / {len(l2['wgrad'])} (second)")
    assert l1["dgrad"] and l1["wgrad"] and l2["dgrad"] and l2["wgrad"]
    assert l3 == l1
    assert set(g3) == set(g1)
    for k, a in g1.items():
        assert float((g3[k] - a).abs().max()) <= BOUND[order[0]] * float(a.abs().max()), k
