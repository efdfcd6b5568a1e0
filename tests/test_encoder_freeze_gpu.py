"""Fine-tuning with the encoder on running statistics and / or frozen weights (``model.encoder``), on the HIP path,
against a CPU torch loop of the oracle network where numbers are involved.  128x128, B = 2."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR = 3e-4


def _pair(seed=0):
    from deadtrees_amd.network.unet import UNetHIP
    from oracle.unet_ref import make_oracle
    ref = make_oracle(3, 2, seed=seed)
    m = UNetHIP()
    m.load_state_dict(ref.state_dict())
    return ref, m.to(DEV)


def _batch(seed=7):
    from deadtrees_amd.data.synthetic import synth_batch
    return synth_batch(2, 128, 128, 3, 2, seed=seed)


class _CpuLoop:
    """the reference's step (Adam + clip_grad_norm_(0.5)) with the encoder in eval mode and / or without gradients;
    not RefTrainer: that one calls model.train() every step"""

    def __init__(self, ref, enc_eval: bool):
        self.ref, self.enc_eval = ref, enc_eval
        self.opt = torch.optim.Adam(ref.parameters(), lr=LR)

    def step(self, img, mask, enc_grad: bool = True):
        from oracle.train_ref import loss_from_logits
        ref = self.ref
        ref.train()
        if self.enc_eval:
            ref.encoder.eval()
        ref.encoder.requires_grad_(enc_grad)
        self.opt.zero_grad(set_to_none=True)
        loss, _ = loss_from_logits(ref(img), mask, ("GDICE", "FOCAL"))
        loss.backward()
        gn = torch.nn.utils.clip_grad_norm_([p for p in ref.parameters() if p.grad is not None], 0.5)
        self.opt.step()
        return float(loss), float(gn)


def _enc_bn(m):
    nb = sum(c.cout for c in m.spec.convs if c.bn_key is not None and c.key.startswith("encoder."))
    return m.bn_state.detach()[:2 * nb].clone(), m.bn_state.detach()[2 * nb:].clone()


def test_encoder_eval_trainable_matches_cpu_loop():
    """MultiStage's effective stage: encoder BatchNorm on running statistics, encoder weights still training"""
    from deadtrees_amd.trainer import HipTrainer
    ref, m = _pair()
    img, mask = _batch()
    m.encoder.eval()
    enc0, dec0 = _enc_bn(m)
    nbt0 = m.num_batches_tracked.clone()
    ht, cpu = HipTrainer(m), _CpuLoop(ref, enc_eval=True)
    for step in range(4):
        lr_, gn_ = cpu.step(img, mask)
        lh = float(ht.step(img.to(DEV), mask.to(DEV)))
        assert m.training and not m.encoder.training            # the trainer keeps the encoder's eval mode
        assert lh == pytest.approx(lr_, rel=5e-3 if step else 2e-5), (step, lh, lr_)
        assert float(ht.last["grad_norm"]) == pytest.approx(gn_, rel=5e-2), step
    enc1, dec1 = _enc_bn(m)
    assert torch.equal(enc0, enc1)                  # running statistics of the encoder: bit-unchanged
    assert not torch.equal(dec0, dec1)              # the decoder's are updated
    n_enc = m._n_enc_convs
    assert torch.equal(m.num_batches_tracked[:n_enc], nbt0[:n_enc])
    assert int(m.num_batches_tracked[-2] - nbt0[-2]) == 4
    sd, sr = m.state_dict(), ref.state_dict()
    for k in ("encoder.layer3.0.conv1.weight", "decoder.blocks.2.conv1.0.weight"):
        assert float((sd[k].cpu() - sr[k]).abs().mean()) < 0.1 * 4 * LR, k


def _no_encoder_launch(eng):
    for kind in ("dgrad", "wgrad"):
        assert eng.launches[kind], kind
        assert not [k for k in eng.launches[kind] if k.startswith("encoder.")], (kind, eng.launches[kind])
    assert "decoder.blocks.0.conv1.0.weight" not in eng.launches["dgrad"]
    assert "decoder.blocks.0.conv1.0.weight" in eng.launches["wgrad"]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_frozen_encoder_eager(precision):
    from deadtrees_amd.trainer import HipTrainer
    ref, m = _pair()
    img, mask = _batch()
    m.encoder.eval()
    m.encoder.requires_grad_(False)
    hi = m.encoder_hi
    p0 = m.flat_params.detach()[:hi].clone()
    enc0, _ = _enc_bn(m)
    ht = HipTrainer(m, precision=precision)
    cpu = _CpuLoop(ref, enc_eval=True)
    for step in range(4):
        lh = float(ht.step(img.to(DEV), mask.to(DEV)))
        _no_encoder_launch(m.engine)
        if precision == "fp32":
            lr_, _ = cpu.step(img, mask, enc_grad=False)
            assert lh == pytest.approx(lr_, rel=5e-3 if step else 2e-5), (step, lh, lr_)
    assert torch.equal(m.flat_params.detach()[:hi], p0)
    assert torch.equal(_enc_bn(m)[0], enc0)
    assert not ht.opt.m[:hi].any() and not ht.opt.v[:hi].any()
    assert ht.opt.v[hi:].any()


def test_frozen_gradients_equal_encoder_eval_gradients():
    """decoder and head gradients of one frozen step = those of the encoder-eval step on the same state and batch"""
    from deadtrees_amd.loss.seg_loss import seg_loss
    ref, _ = _pair()
    img, mask = _batch()
    grads = {}
    for frozen in (False, True):
        from deadtrees_amd.network.unet import UNetHIP
        m = UNetHIP()
        m.load_state_dict(ref.state_dict())
        m.to(DEV).train()
        m.encoder.eval()
        m.encoder.requires_grad_(not frozen)
        m.flat_params.grad = None
        logits = m(img.to(DEV))
        loss, _, _ = seg_loss(logits, mask.to(DEV), None, ("GDICE", "FOCAL"))
        loss.backward()
        grads[frozen] = m.smp_grad_dict()
        if frozen:      # the autograd path: nothing in the encoder slice
            assert not m.flat_params.grad[:m.encoder_hi].any()
    for k, g in grads[False].items():
        if k.startswith("encoder."):
            continue
        gf = grads[True][k]
        rel = float((gf.double() - g.double()).norm() / g.double().norm().clamp_min(1e-30))
        assert rel <= 1e-6, (k, rel)


def test_freeze_then_unfreeze_matches_cpu_loop():
    """2 frozen steps, then 2 with the encoder trainable: the encoder's first update uses the step-1 bias correction
    (its own step count), as torch.optim.Adam after steps where the encoder's .grad was None"""
    from deadtrees_amd.trainer import HipTrainer
    ref, m = _pair()
    img, mask = _batch()
    ht, cpu = HipTrainer(m), _CpuLoop(ref, enc_eval=False)
    for step in range(4):
        frozen = step < 2
        m.encoder.requires_grad_(not frozen)
        lr_, gn_ = cpu.step(img, mask, enc_grad=not frozen)
        lh = float(ht.step(img.to(DEV), mask.to(DEV)))
        assert lh == pytest.approx(lr_, rel=5e-3 if step else 2e-5), (step, lh, lr_)
        assert float(ht.last["grad_norm"]) == pytest.approx(gn_, rel=5e-2), step
    sd, sr = m.state_dict(), ref.state_dict()
    k = "decoder.blocks.2.conv1.0.weight"
    assert float((sd[k].cpu() - sr[k]).abs().mean()) < 0.1 * 4 * LR, k
    # the encoder's Adam step count started at its first update (the bias correction itself: test below)
    t = ht.opt.t_seg.cpu().tolist()
    assert t == [2.0, 4.0], t


def test_flat_adam_ranges_match_torch_adam():
    """FlatAdam.set_trainable against torch.optim.Adam where the frozen tensor's .grad is None: clip over the
    trainable part, per-range step counts (step-1 bias correction at the first update after a freeze), reset_state"""
    from deadtrees_amd.ops import FlatAdam
    g = torch.Generator().manual_seed(0)
    n, hi = 4096 + 64, 1024
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) for _ in range(6)]
    a, b = torch.nn.Parameter(p0[:hi].clone()), torch.nn.Parameter(p0[hi:].clone())
    ref = torch.optim.Adam([a, b], lr=1e-2)
    flat = p0.clone().to(DEV)
    opt = FlatAdam(flat, lr=1e-2, max_norm=0.5)
    for step, gr in enumerate(grads):
        if step == 4:
            ref = torch.optim.Adam([a, b], lr=1e-2 / 3)          # the LR-reduce stage: a fresh optimiser
            opt.reset_state(lr=1e-2 / 3)
        frozen = step < 2
        opt.set_trainable([(hi, n)] if frozen else None)
        a.grad = None if frozen else gr[:hi].clone()
        b.grad = gr[hi:].clone()
        gn = torch.nn.utils.clip_grad_norm_([p for p in (a, b) if p.grad is not None], 0.5)
        ref.step()
        gd = gr.to(DEV)
        gd[:hi] = float("nan") if frozen else gd[:hi]            # a frozen range is never read
        norm = opt.step(gd)
        assert float(norm) == pytest.approx(float(gn), rel=1e-5), step
        got = flat.cpu()
        torch.testing.assert_close(got[:hi], a.detach(), rtol=0, atol=2e-6)
        torch.testing.assert_close(got[hi:], b.detach(), rtol=0, atol=2e-6)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_frozen_graph_equals_eager_with_toggle(precision):
    from deadtrees_amd.trainer import HipTrainer
    ref, _ = _pair()
    img, mask = (t.to(DEV) for t in _batch())
    out = {}
    for mode in ("eager", "graph"):
        from deadtrees_amd.network.unet import UNetHIP
        m = UNetHIP()
        m.load_state_dict(ref.state_dict())
        m.to(DEV)
        tr = HipTrainer(m, precision=precision, graph=(mode == "graph"))
        losses = []
        for step in range(8):
            m.encoder.requires_grad_(step >= 4)      # frozen for 4 steps, then trainable: a re-capture
            losses.append(float(tr.step(img, mask)))
        if mode == "graph":
            assert "graph" in tr._graph and tr._graph["key"][-2] is False
        out[mode] = (losses, m.flat_params.detach().clone(), tr.opt.m.clone(), m.bn_state.clone())
    le, pe, me, be = out["eager"]
    lg, pg, mg, bg = out["graph"]
    assert le == lg
    assert torch.equal(pe, pg) and torch.equal(me, mg) and torch.equal(be, bg)


def test_frozen_nan_loss_skips_update():
    from deadtrees_amd.trainer import HipTrainer
    _, m = _pair()
    img, mask = _batch()
    m.encoder.eval()
    m.encoder.requires_grad_(False)
    ht = HipTrainer(m)
    ht.step(img.to(DEV), mask.to(DEV))
    before = m.flat_params.detach().clone()
    bad = img.clone()
    bad[0, 0, 0, 0] = float("nan")
    ht.step(bad.to(DEV), mask.to(DEV))
    assert int(ht.last["skipped"]) == 1
    assert torch.equal(m.flat_params.detach(), before)
    ht.step(img.to(DEV), mask.to(DEV))
    assert int(ht.last["skipped"]) == 0
    assert not torch.equal(m.flat_params.detach()[m.encoder_hi:], before[m.encoder_hi:])
