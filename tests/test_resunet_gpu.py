"""architecture "resunet" (the reference's in-tree ResUnet, deadtrees/network/segmodel.py:66-67 ->
network/extra/resunet/{model,decoder}.py) on the HIP kernels, against oracle/resunet_ref.py — whose decoder is pinned
by the executed reference (tests/golden/resunet_decoder.part*.npz, tests/test_oracle_golden.py)."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _pair(C=3, K=2, seed=0):
    from deadtrees_amd.network.unet import UNetHIP
    from oracle.resunet_ref import make_resunet_oracle
    ref = make_resunet_oracle(C, K, seed=seed)
    m = UNetHIP(in_channels=C, classes=K, decoder="resunet")
    m.load_state_dict(ref.state_dict())
    return ref, m.to(DEV)


@pytest.mark.parametrize("B,H,W,C,K", [(2, 64, 64, 3, 2), (1, 128, 160, 4, 3)])
def test_resunet_forward_eval_parity_and_argmax(B, H, W, C, K):
    from deadtrees_amd.data.synthetic import synth_batch
    ref, m = _pair(C, K)
    img, _ = synth_batch(B, H, W, C, K, seed=5)
    ref.eval()
    m.eval()
    with torch.no_grad():
        want64 = copy.deepcopy(ref).double()(img.double())
        got = m(img.to(DEV)).cpu()
    scale, err = float(want64.abs().max()), float((got.double() - want64).abs().max())
    assert err <= 1e-4 * scale, (err, scale)
    top2 = want64.topk(2, dim=1).values
    safe = (top2[:, 0] - top2[:, 1]) > 4 * err
    am = m.predict_classes(img.to(DEV)).cpu()
    assert torch.equal(am, got.argmax(dim=1)) and torch.equal(am[safe], want64.argmax(dim=1)[safe])


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_resunet_training_step_gradients(mode):
    """loss and every parameter gradient (incl. the 1x1 identity convolutions, their biases and the 1x1 head) against
    the fp64 oracle.  The residual decoder has no normalisation after its sums, so its logits carry the fp32
    accumulation error of long 1x1 / 3x3 channel sums un-normalised (measured: 3.5e-6 relative L2, 1e-5 of max|logit|,
    about 3x torch's blocked CPU sums) and d loss / d logits amplifies that into ~5e-4 of every gradient.  The test
    therefore separates the two halves: (a) logits and loss against the oracle; (b) the BACKWARD pass against the
    oracle's backward driven by the SAME upstream gradient (the HIP path's own d loss / d logits); (c) end to end,
    a loose bound.  Measured for (b) with frozen BatchNorm (scripts/diag_resunet.py): head, identity convolutions and
    the last decoder block agree to 3e-7; from there a handful of ReLU masks of pre-activations within ~1e-6 of zero
    differ from the oracle's (the MFMA's sequential fp32 channel sums are ~10x less accurate than oneDNN's blocked
    ones, so more elements sit on the other side of zero) and every flipped element changes a gradient by its full
    value: 1e-4 .. 8e-4 per tensor further down — the same effect the plain U-Net shows (3e-4).  A wiring error
    (wrong operand, missing residual / bias term) is O(0.1 .. 1).  Bounds: 2e-3 per tensor frozen, the fp32-CPU
    yardstick x 6 with batch statistics."""
    from deadtrees_amd.data.synthetic import synth_batch
    from deadtrees_amd.loss.seg_loss import seg_loss
    from oracle.train_ref import loss_from_logits
    ref, m = _pair(3, 2, seed=3)
    img, mask = synth_batch(2, 128, 128, 3, 2, seed=6)
    ref64, ref32, ref64e = copy.deepcopy(ref).double(), copy.deepcopy(ref), copy.deepcopy(ref).double()
    for mod in (ref64, ref32, ref64e, m):
        mod.train(mode == "train")
    logits = m(img.to(DEV))
    logits.retain_grad()
    loss, _, _ = seg_loss(logits, mask.to(DEV), None, ("GDICE", "FOCAL"))
    loss.backward()
    dl_hip = logits.grad.detach().cpu()
    l64 = ref64(img.double())
    loss64, _ = loss_from_logits(l64, mask, ("GDICE", "FOCAL"))
    assert float((logits.detach().cpu().double() - l64.detach()).norm() / l64.detach().norm()) <= 2e-5
    assert float(loss.detach()) == pytest.approx(float(loss64.detach()), rel=2e-5)
    l64.backward(dl_hip.double())                       # (b): the oracle's backward for the HIP path's upstream gradient
    l32 = ref32(img)
    l32.backward(dl_hip)
    l64e = ref64e(img.double())                         # (c): end to end
    loss_from_logits(l64e, mask, ("GDICE", "FOCAL"))[0].backward()
    grads = m.smp_grad_dict()
    g32 = {k: p.grad for k, p in ref32.named_parameters()}
    g64e = {k: p.grad for k, p in ref64e.named_parameters()}
    assert set(grads) == {k for k, _ in ref64.named_parameters()}
    gscale = max(float(p.grad.norm()) for p in ref64.parameters())
    worst, worst_e2e = (0.0, ""), (0.0, "")
    for k, p in ref64.named_parameters():
        n = float(p.grad.norm())
        e = float((grads[k].double() - p.grad).norm())
        e32 = float((g32[k].double() - p.grad).norm())
        worst = max(worst, (e / (n + 1e-30), k))
        worst_e2e = max(worst_e2e, (float((grads[k].double() - g64e[k]).norm()) / (float(g64e[k].norm()) + 1e-30), k))
        if mode == "eval":
            assert e <= 2e-3 * n + 1e-7 * gscale, (k, e / n, e32 / n)
            if "blocks.4" in k or "segmentation_head" in k:      # before the first possible mask flip: exact
                assert e <= 5e-6 * n + 1e-7 * gscale, (k, e / n)
        else:
            assert e <= 6.0 * e32 + 1e-3 * n + 1e-7 * gscale, (k, e / n, e32 / n)
    print(f"[resunet {mode}] worst per-tensor gradient rel-L2 vs fp64 oracle: backward alone {worst[0]:.2e} ({worst[1]}), "
          f"end to end {worst_e2e[0]:.2e} ({worst_e2e[1]})")
    assert worst_e2e[0] <= (5e-3 if mode == "eval" else 1e-1)
    if mode == "train":
        sd_ref, sd = ref32.state_dict(), m.state_dict()
        for k in sd_ref:
            if k.endswith("running_mean") or k.endswith("running_var"):
                np.testing.assert_allclose(sd[k].cpu().numpy(), sd_ref[k].numpy(), rtol=2e-4, atol=2e-5, err_msg=k)


def test_resunet_trains_through_semsegment_and_hiptrainer():
    """SemSegment(architecture="resunet") builds the model; HipTrainer steps it (loss falls, head stays 1x1)."""
    from deadtrees.network.segmodel import SemSegment
    from deadtrees_amd.data.synthetic import synth_batch
    from deadtrees_amd.trainer import HipTrainer
    from deadtrees_amd.utils.config import default_network, default_training
    model = SemSegment(default_network(architecture="resunet"), default_training()).to(DEV)
    assert model.model.spec.decoder_kind == "resunet"
    assert tuple(model.model.state_dict()["segmentation_head.0.weight"].shape) == (2, 16, 1, 1)
    img, mask = synth_batch(4, 64, 64, 3, 2, seed=9)
    img[:, 0] += 2.5 * mask.float()
    tr = HipTrainer(model.model, lr=3e-4)
    losses = [float(tr.step(img.to(DEV), mask.to(DEV))) for _ in range(12)]
    assert np.isfinite(losses).all() and min(losses[1:]) < losses[0], losses
    hd = model.model.spec.head
    w = model.model.flat_params.detach()[hd.w_off:hd.w_off + hd.w_size].view(2, 9, 16)
    assert float(w[:, :4].abs().max()) == 0.0 and float(w[:, 5:].abs().max()) == 0.0      # off-centre taps stay zero
    # under AMP (round 3: bf16 forms of the ResUnet decoder — teacher-forced parity in tests/test_bf16_e2e_gpu.py): the same
    # model keeps training, with HIP-graph replay too; the 1x1 head stays 1x1; bf16 inference agrees with fp32 on the class maps
    trb = HipTrainer(model.model, lr=3e-4, precision="bf16", graph=True)
    lb = [float(trb.step(img.to(DEV), mask.to(DEV))) for _ in range(8)]
    assert np.isfinite(lb).all() and lb[-1] < losses[0], lb
    w = model.model.flat_params.detach()[hd.w_off:hd.w_off + hd.w_size].view(2, 9, 16)
    assert float(w[:, :4].abs().max()) == 0.0 and float(w[:, 5:].abs().max()) == 0.0
    model.model.eval()
    a32 = model.model.predict_classes(img.to(DEV), dtype="uint8")
    a16 = model.model.predict_classes(img.to(DEV), dtype="uint8", precision="bf16")
    assert float((a32 == a16).float().mean()) > 0.97
