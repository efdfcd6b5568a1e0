"""Fine-tuning with the encoder on running statistics and / or frozen weights (``model.encoder``), on the HIP path,
against a CPU torch loop of the oracle network where numbers are involved.  128x128, B = 2."""
import numpy as np
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
            (key,), (r,) = tr._step_replays.keys(), tr._step_replays.values()
            assert r.captured and key[-2] is False
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


# ---------------------------------------------------------------- per-tensor gradient parity against fp64 oracles
def _calibrate_encoder(ref, seed=11, C=3):
    """calibrated encoder running statistics: a few train-mode forwards with momentum=None (a cumulative average) on
    other synthetic batches, momentum back to 0.1 (the decoder's running-statistics check depends on it), then spread
    per channel — running_var x log-uniform[0.5, 2], running_mean + 0.3 std — so eval-mode BatchNorm is far from the
    identity while the logits stay O(10)"""
    from deadtrees_amd.data.synthetic import synth_batch
    bns = [mod for mod in ref.encoder.modules() if isinstance(mod, torch.nn.BatchNorm2d)]
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in bns:
            mod.reset_running_stats()
            mod.momentum = None
        ref.train()
        for i in range(3):
            ref(synth_batch(2, 128, 128, C, 2, seed=seed + 100 + i)[0])
        for mod in bns:
            mod.momentum = 0.1
            c = mod.running_var.numel()
            mod.running_var.mul_(torch.exp(torch.empty(c).uniform_(float(np.log(0.5)), float(np.log(2.0)), generator=g)))
            mod.running_mean.add_(0.3 * mod.running_var.sqrt() * torch.randn(c, generator=g))
            mod.num_batches_tracked.fill_(3)
    return ref


def _calibrated_pair(C=3, K=2, seed=0, tmp_path=None):
    """(oracle, HIP model) with calibrated encoder statistics; tmp_path given: the HIP model's encoder is loaded from a
    torchvision-named .pth of the oracle's encoder (UNetHIP(encoder_weights=...)), its decoder and head (smp init) are
    copied into the oracle — a mix-up of the loader's key mapping then shows in every number"""
    from deadtrees_amd.network.unet import UNetHIP
    from oracle.unet_ref import make_oracle
    ref = _calibrate_encoder(make_oracle(C, K, seed=seed), C=C)
    if tmp_path is None:
        m = UNetHIP(in_channels=C, classes=K)
        m.load_state_dict(ref.state_dict())
        return ref, m.to(DEV)
    sd = {k[len("encoder."):]: v.clone() for k, v in ref.state_dict().items() if k.startswith("encoder.")}
    sd["fc.weight"], sd["fc.bias"] = torch.zeros(1000, 512), torch.zeros(1000)
    path = tmp_path / "resnet34_tv.pth"
    torch.save(sd, path)
    with torch.random.fork_rng(devices=[]):       # smp's decoder init draws from the global generator
        torch.manual_seed(seed)
        m = UNetHIP(in_channels=C, classes=K, encoder_weights=str(path))
    rs = ref.state_dict()
    ref.load_state_dict({k: (rs[k] if k.startswith("encoder.") else v.cpu()) for k, v in m.state_dict().items()})
    return ref, m.to(DEV)


def _oracle_step(ref, img, mask, names, dist, enc_eval, frozen):
    from oracle.train_ref import loss_from_logits
    ref.train()
    if enc_eval:
        ref.encoder.eval()
    ref.encoder.requires_grad_(not frozen)
    dt = next(ref.parameters()).dtype
    logits = ref(img.to(dt))
    loss, _ = loss_from_logits(logits, mask, names, None if dist is None else dist.to(dt))
    loss.backward()
    return logits.detach(), loss.detach()


def _dist(mask, K, names):
    from oracle.losses_ref import dist_map, one_hot
    if "BOUNDARY" not in names:
        return None
    oh = one_hot(mask, K).numpy()
    return torch.from_numpy(np.stack([dist_map(oh[i]) for i in range(mask.shape[0])]).astype(np.float32))


FLIP_PRONE = ("decoder.blocks.3.", "decoder.blocks.4.")     # the two highest-resolution decoder blocks


def _grad_parity(m, ref, ref64, winograd, skip_encoder, tag):
    """test_train_step_gradient_parity's yardstick: per tensor, the HIP gradient's distance from fp64 <= N x the fp32
    CPU oracle's own + 1e-4 |g|; over all tensors the same with the overall factor.  -> (worst ratio, its tensor).
    Only the tensors of decoder blocks 3 and 4 get a floor of 5e-4 |g|: with the encoder on calibrated running
    statistics the HIP forward folds BatchNorm into scale / shift (the frozen encoder: into the convolution's
    epilogue), torch normalises; the few ReLU masks this flips at the highest resolutions moved single small tensors
    there by up to 4e-4 |g| (measured: decoder.blocks.4.conv1.1.weight, |g| = 0.009; decoder.blocks.4.conv2.0.weight
    1.6e-4) while the fp32 CPU oracle flipped none of them.  The report quotes the worst ratio at the 1e-4 floor."""
    from conftest import parity_report
    per_tensor, overall = (10.0, 5.0) if winograd else (4.0, 2.0)
    grads = m.smp_grad_dict()
    g32 = {k: p.grad for k, p in ref.named_parameters()}
    g64 = {k: p.grad for k, p in ref64.named_parameters()}
    tot_hip = tot_ref = tot = 0.0
    worst, worst_k, worst4, worst4_k = 0.0, None, 0.0, None
    for k, g in g64.items():
        if skip_encoder and k.startswith("encoder."):
            assert g is None and g32[k] is None, k
            continue
        n = float(g.norm()) + 1e-30
        eh = float((grads[k].double() - g).norm())
        er = float((g32[k].double() - g).norm())
        floor = 5e-4 if k.startswith(FLIP_PRONE) else 1e-4
        assert eh <= per_tensor * er + floor * n, (k, eh / n, er / n)
        ratio, ratio4 = eh / (per_tensor * er + floor * n), eh / (per_tensor * er + 1e-4 * n)
        if ratio > worst:
            worst, worst_k = ratio, k
        if ratio4 > worst4:
            worst4, worst4_k = ratio4, k
        tot_hip += eh ** 2
        tot_ref += er ** 2
        tot += n ** 2
    assert tot_hip ** 0.5 <= overall * tot_ref ** 0.5 + 1e-5 * tot ** 0.5, (tot_hip, tot_ref, tot)
    parity_report(f"{tag}: worst per-tensor err / bound {worst:.3f} ({worst_k}); at the 1e-4 floor everywhere "
                  f"{worst4:.3f} ({worst4_k}); overall err / fp32 err {(tot_hip / max(tot_ref, 1e-300)) ** 0.5:.2f} "
                  f"(bound {overall})")
    return worst, worst_k


def _logits_loss_parity(logits, loss, lref, l64, loss64):
    e_hip = float((logits.detach().cpu().double() - l64).abs().max())
    e_ref = float((lref.double() - l64).abs().max())
    assert e_hip <= max(3 * e_ref, 1e-4 * float(l64.abs().max())), (e_hip, e_ref)
    assert float(loss.detach()) == pytest.approx(float(loss64), rel=2e-5)
    assert float(l64.abs().max()) < 50.0        # calibrated statistics: logits stay O(10)


PARITY_CASES = [  # C, K, losses, Winograd engine, how the HIP model gets its encoder
    (3, 2, ("GDICE", "FOCAL"), False, "state_dict"), (4, 3, ("DICE", "FOCAL", "BOUNDARY"), False, "state_dict"),
    (3, 2, ("GDICE", "FOCAL"), True, "state_dict"), (4, 3, ("DICE", "FOCAL", "BOUNDARY"), True, "state_dict"),
    (3, 2, ("GDICE", "FOCAL"), True, "torchvision_pth")]


@pytest.mark.parametrize("C,K,names,winograd,load", PARITY_CASES)
def test_encoder_eval_trainable_gradient_parity(C, K, names, winograd, load, tmp_path):
    """encoder BatchNorm on (calibrated, wide) running statistics, all weights trainable: one step, every parameter
    gradient against an fp64 oracle in the same mode (ref.train(); ref.encoder.eval()), logits, loss, the decoder's
    running statistics updated like torch's, the encoder's and its num_batches_tracked bit-unchanged"""
    import copy
    from deadtrees_amd.data.distmap import distmaps_on_device
    from deadtrees_amd.loss.seg_loss import seg_loss
    ref, m = _calibrated_pair(C, K, tmp_path=tmp_path if load == "torchvision_pth" else None)
    m.engine.winograd = winograd
    ref64 = copy.deepcopy(ref).double()
    img, mask = _synth_ck(C, K)
    dist = _dist(mask, K, names)
    lref, _ = _oracle_step(ref, img, mask, names, dist, enc_eval=True, frozen=False)
    l64, loss64 = _oracle_step(ref64, img, mask, names, dist, enc_eval=True, frozen=False)
    m.train()
    m.encoder.eval()
    enc0, _ = _enc_bn(m)
    nbt0 = m.num_batches_tracked.clone()
    logits = m(img.to(DEV))
    ddist = distmaps_on_device(mask.to(DEV), K) if dist is not None else None
    loss, _, err = seg_loss(logits, mask.to(DEV), ddist, names)
    loss.backward()
    assert int(err) == 0
    _logits_loss_parity(logits, loss, lref, l64, loss64)
    _grad_parity(m, ref, ref64, winograd, False, f"encoder eval, trainable C={C} K={K} wino={winograd} {load}")
    sd_ref, sd = ref.state_dict(), m.state_dict()
    for k in sd_ref:
        if k.startswith("decoder.") and (k.endswith("running_mean") or k.endswith("running_var")):
            np.testing.assert_allclose(sd[k].cpu().numpy(), sd_ref[k].numpy(), rtol=2e-4, atol=2e-5, err_msg=k)
    enc1, _ = _enc_bn(m)
    assert torch.equal(enc0, enc1)
    n_enc = m._n_enc_convs
    assert torch.equal(m.num_batches_tracked[:n_enc], nbt0[:n_enc])
    assert torch.equal(m.flat_params.grad, m._grad_buffer())


def _synth_ck(C, K, B=2, H=128, W=128, seed=1234):
    from deadtrees_amd.data.synthetic import synth_batch
    return synth_batch(B, H, W, C, K, seed)


@pytest.mark.parametrize("enc_eval,winograd", [(True, False), (True, True), (False, True)])
def test_frozen_encoder_gradient_parity(enc_eval, winograd):
    """frozen encoder weights, encoder in eval mode (the fused inference form) or train mode (batch statistics, running
    statistics updated like torch's): decoder and head gradients per tensor against fp64, the encoder slice of .grad
    and of the gradient buffer exactly zero, the 9 data / 10 weight gradients of DESIGN section 11 (either engine) and
    none of the encoder"""
    import copy
    from deadtrees_amd.loss.seg_loss import seg_loss
    names = ("GDICE", "FOCAL")
    ref, m = _calibrated_pair()
    m.engine.winograd = winograd
    ref64 = copy.deepcopy(ref).double()
    img, mask = _batch()
    lref, _ = _oracle_step(ref, img, mask, names, None, enc_eval=enc_eval, frozen=True)
    l64, loss64 = _oracle_step(ref64, img, mask, names, None, enc_eval=enc_eval, frozen=True)
    m.train()
    if enc_eval:
        m.encoder.eval()
    m.encoder.requires_grad_(False)
    m.flat_params.grad = None
    enc0, _ = _enc_bn(m)
    logits = m(img.to(DEV))
    loss, _, _ = seg_loss(logits, mask.to(DEV), None, names)
    loss.backward()
    _logits_loss_parity(logits, loss, lref, l64, loss64)
    eng = m.engine
    _no_encoder_launch(eng)
    n_d, n_w = len(eng.launches["dgrad"]), len(eng.launches["wgrad"])
    assert (n_d, n_w) == (9, 10), (eng.launches["dgrad"], eng.launches["wgrad"])     # both engines
    _grad_parity(m, ref, ref64, winograd, True,
                 f"frozen encoder ({'eval' if enc_eval else 'train'}) wino={winograd}: dgrad {n_d} wgrad {n_w}")
    hi = m.encoder_hi
    assert not m.flat_params.grad[:hi].any() and not m._grad_buffer()[:hi].any()
    sd_ref, sd = ref.state_dict(), m.state_dict()
    for k in sd_ref:
        if k.endswith("running_mean") or k.endswith("running_var"):
            np.testing.assert_allclose(sd[k].cpu().numpy(), sd_ref[k].numpy(), rtol=2e-4, atol=2e-5, err_msg=k)
    if enc_eval:
        assert torch.equal(_enc_bn(m)[0], enc0)


def test_frozen_equals_encoder_eval_gradients_at_bench_shape():
    """B=32, 512x512, fp32 Winograd (the benchmark's shape; no CPU oracle): decoder and head gradients of the frozen step
    equal the encoder-eval step's to 5e-6 relative L2 — the network-level run of the narrowed data gradient with several
    tiles per workgroup (8 / 16 / 32 in decoder blocks 1 / 2 / 3).  Not 1e-6 as at 128x128: the two steps' encoder
    forwards differ in rounding (the frozen one is the fused inference form), measured 1.8e-6 on decoder.blocks.0's
    conv1 weight, whose input is the encoder's output"""
    from deadtrees_amd.loss.seg_loss import seg_loss
    from deadtrees_amd.network.unet import UNetHIP
    from oracle.unet_ref import make_oracle
    from conftest import parity_report
    ref = _calibrate_encoder(make_oracle(3, 2, seed=0))
    img, mask = _synth_ck(3, 2, B=32, H=512, W=512, seed=21)
    img, mask = img.to(DEV), mask.to(DEV)
    grads = {}
    for frozen in (False, True):
        m = UNetHIP()
        m.load_state_dict(ref.state_dict())
        m.to(DEV).train()
        m.encoder.eval()
        m.encoder.requires_grad_(not frozen)
        assert m.engine.winograd
        m.flat_params.grad = None
        loss, _, _ = seg_loss(m(img), mask, None, ("GDICE", "FOCAL"))
        loss.backward()
        grads[frozen] = {k: v.clone() for k, v in m.smp_grad_dict().items() if not k.startswith("encoder.")}
        del m, loss
    worst, worst_k = 0.0, None
    for k, g in grads[False].items():
        gf = grads[True][k]
        rel = float((gf.double() - g.double()).norm() / g.double().norm().clamp_min(1e-30))
        assert rel <= 5e-6, (k, rel)
        if rel >= worst:
            worst, worst_k = rel, k
    parity_report(f"frozen vs encoder-eval gradients B=32 512x512: worst relative L2 {worst:.2e} ({worst_k})")


@pytest.mark.parametrize("frozen", [False, True])
def test_unetpp_encoder_eval_and_frozen_gradient_parity(frozen):
    """Unet++ decoder, fp32, encoder on calibrated running statistics with trainable or frozen weights, against
    make_unetpp_oracle in the same mode.  (a) logits within 1e-4 of max|logit| and the loss at rel 2e-5 against fp64;
    (b) the backward pass against the fp64 and fp32 oracles' backward driven by the SAME upstream gradient (the HIP
    path's own d loss / d logits), per tensor within 10x the fp32 CPU oracle's distance from fp64 + 1e-3 |g| (a flipped
    ReLU mask moves a tensor of this decoder by ~1e-3: the floor of its own batch-statistics test; measured worst 0.40
    of the bound), 5x overall; frozen: no encoder gradient, the encoder slice of .grad exactly zero.  Decoder running
    statistics as torch's, the encoder's bit-unchanged."""
    import copy
    from deadtrees_amd.loss.seg_loss import seg_loss
    from deadtrees_amd.network.unet import UNetHIP
    from oracle.train_ref import loss_from_logits
    from oracle.unetpp_ref import make_unetpp_oracle
    from conftest import parity_report
    names = ("GDICE", "FOCAL")
    ref = _calibrate_encoder(make_unetpp_oracle(3, 2, seed=3))
    m = UNetHIP(in_channels=3, classes=2, decoder="unetplusplus")
    m.load_state_dict(ref.state_dict())
    m.to(DEV)
    img, mask = _batch()
    ref64, ref32 = copy.deepcopy(ref).double(), copy.deepcopy(ref)
    for mod in (ref64, ref32, m):
        mod.train()
        mod.encoder.eval()
        mod.encoder.requires_grad_(not frozen)
    enc0, _ = _enc_bn(m)
    m.flat_params.grad = None
    logits = m(img.to(DEV))
    logits.retain_grad()
    loss, _, _ = seg_loss(logits, mask.to(DEV), None, names)
    loss.backward()
    dl = logits.grad.detach().cpu()
    l64 = ref64(img.double())
    loss64, _ = loss_from_logits(l64, mask, names)
    e = float((logits.detach().cpu().double() - l64.detach()).abs().max())
    assert e <= 1e-4 * float(l64.detach().abs().max()), e
    assert float(l64.detach().abs().max()) < 50.0
    assert float(loss.detach()) == pytest.approx(float(loss64.detach()), rel=2e-5)
    l64.backward(dl.double())
    ref32(img).backward(dl)
    grads = m.smp_grad_dict()
    g32 = {k: p.grad for k, p in ref32.named_parameters()}
    tot_h = tot_r = tot = 0.0
    worst, worst_k = 0.0, None
    for k, p in ref64.named_parameters():
        if frozen and k.startswith("encoder."):
            assert p.grad is None and g32[k] is None, k
            continue
        n = float(p.grad.norm()) + 1e-30
        eh = float((grads[k].double() - p.grad).norm())
        er = float((g32[k].double() - p.grad).norm())
        assert eh <= 10.0 * er + 1e-3 * n, (k, eh / n, er / n)
        if eh / (10.0 * er + 1e-3 * n) > worst:
            worst, worst_k = eh / (10.0 * er + 1e-3 * n), k
        tot_h += eh ** 2
        tot_r += er ** 2
        tot += n ** 2
    assert tot_h ** 0.5 <= 5.0 * tot_r ** 0.5 + 1e-5 * tot ** 0.5, (tot_h, tot_r, tot)
    parity_report(f"unet++ encoder {'frozen' if frozen else 'eval, trainable'}: worst per-tensor err / bound "
                  f"{worst:.3f} ({worst_k}), overall err / fp32 err {(tot_h / max(tot_r, 1e-300)) ** 0.5:.2f} (bound 5)")
    if frozen:
        assert not m.flat_params.grad[:m.encoder_hi].any()
    sd_ref, sd = ref32.state_dict(), m.state_dict()
    for k in sd_ref:
        if k.startswith("decoder.") and (k.endswith("running_mean") or k.endswith("running_var")):
            np.testing.assert_allclose(sd[k].cpu().numpy(), sd_ref[k].numpy(), rtol=2e-4, atol=2e-5, err_msg=k)
    assert torch.equal(_enc_bn(m)[0], enc0)


def test_bf16_encoder_eval_with_trainable_weights_raises():
    """bf16 has no frozen-statistics BatchNorm backward: an eval-mode encoder with trainable weights is refused before
    anything runs, and nothing changes"""
    from deadtrees_amd.trainer import HipTrainer
    _, m = _pair()
    img, mask = _batch()
    m.encoder.eval()
    p0, b0 = m.flat_params.detach().clone(), m.bn_state.detach().clone()
    ht = HipTrainer(m, precision="bf16")
    with pytest.raises(NotImplementedError):
        ht.step(img.to(DEV), mask.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(m.flat_params.detach(), p0) and torch.equal(m.bn_state.detach(), b0)
