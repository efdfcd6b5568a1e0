"""Inference, training and recalibration passes of both precisions interleaved on ONE engine object.  All of them run
through one forward schedule with per-pass state — the BatchNorm mode of the pass, the fused inference forms switched on
for a frozen eval-mode encoder, the recalibration momentum of a pass that ends early, the cache of eval-mode BatchNorm
coefficients — and none of that state may reach the next pass.

Per trainable decoder kind, one ``UNetHIP`` runs: fp32 prediction, bf16 prediction, a bf16 trainer step, fp32 prediction,
an fp32 recalibration batch, bf16 prediction, an fp32 trainer step with the encoder frozen and in eval mode, fp32
``predict_logits``, a bf16 recalibration batch, the fp32 fused evaluation head.  After every inference call a second model
that has run nothing else receives the first one's parameters and ``bn_state`` as they are at that moment and makes the
same call: class maps and confusion counts are equal, logits bit-equal (they are: inference at these shapes launches no
atomics, and a stale coefficient, a wrong BatchNorm mode or a fused form left on would move them far beyond rounding).
2 x 64 x 64 on ``synth_batch``; about a second per decoder kind.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _model(kind):
    from deadtrees_amd.network.unet import UNetHIP
    m = UNetHIP(in_channels=3, classes=2, decoder=kind)
    m.reset_parameters(seed=0)
    return m.to(DEV).train()


def _fresh_copy(m, kind):
    """a model that has run nothing, with m's parameters and BatchNorm state of this moment"""
    f = _model(kind)
    with torch.no_grad():
        f.flat_params.data.copy_(m.flat_params.data)
        f.bn_state.copy_(m.bn_state)
    return f


def _check_prediction(m, kind, img, precision, what):
    f = _fresh_copy(m, kind)
    cls, logits = m.predict_classes(img, precision=precision), m.predict_logits(img, precision=precision)
    cls_f, logits_f = f.predict_classes(img, precision=precision), f.predict_logits(img, precision=precision)
    torch.cuda.synchronize()
    diff = float((logits - logits_f).abs().max())
    print(f"[interleaved {kind}] {what}: {precision} logits max|a - fresh| = {diff:.3e} of max|fresh| = "
          f"{float(logits_f.abs().max()):.3e}, class maps differ in {int((cls != cls_f).sum())} pixels")
    assert torch.isfinite(logits_f).all()
    assert torch.equal(cls, cls_f), what
    assert torch.equal(logits, logits_f), what


@pytest.mark.parametrize("kind", ["unet", "resunet", "unetplusplus"])
def test_no_pass_leaves_state_to_the_next(kind):
    from deadtrees_amd.data.synthetic import synth_batch
    from deadtrees_amd.trainer import HipTrainer
    m = _model(kind)
    eng = m.engine
    img, mask = synth_batch(2, 64, 64, 3, 2, seed=4321)
    img, mask = img.to(DEV), mask.to(DEV)

    _check_prediction(m, kind, img, "fp32", "1 first call")
    _check_prediction(m, kind, img, "bf16", "2 after an fp32 prediction")
    HipTrainer(m, precision="bf16").step(img, mask)
    _check_prediction(m, kind, img, "fp32", "4 after a bf16 training step")
    m.recalibrate_batch(img, "fp32")
    _check_prediction(m, kind, img, "bf16", "6 after an fp32 recalibration batch")
    m.encoder.requires_grad_(False)
    m.encoder.eval()
    HipTrainer(m, precision="fp32").step(img, mask)
    f = _fresh_copy(m, kind)
    logits, logits_f = m.predict_logits(img), f.predict_logits(img)
    print(f"[interleaved {kind}] 8 after an fp32 step on a frozen eval-mode encoder: max|a - fresh| = "
          f"{float((logits - logits_f).abs().max()):.3e}")
    assert torch.equal(logits, logits_f)
    m.recalibrate_batch(img, "bf16")
    f = _fresh_copy(m, kind)
    got = eng.forward_eval_head(img, m.flat_params.detach(), m.bn_state, mask, want_argmax=True)
    ref = f.engine.forward_eval_head(img, f.flat_params.detach(), f.bn_state, mask, want_argmax=True)
    torch.cuda.synchronize()
    assert m.engine is eng
    assert int(got[3]) == 0 and int(ref[3]) == 0
    assert int(got[1].sum()) > 0
    assert torch.equal(got[1], ref[1])          # confusion counts
    assert torch.equal(got[2], ref[2])          # class map
    assert eng._recal is None
