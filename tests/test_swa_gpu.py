"""Stochastic weight averaging on the MI355X: the averaging kernel, the device-momentum BatchNorm finalize, the
statistics-only recalibration forward (``update_bn``) against ``torch.optim.swa_utils`` on the CPU oracles, graph replay,
EMA inside the training step and ``fit(swa=...)`` end to end.  Needs an MI355X."""
import copy
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 4096            # NaN floats on both sides of avg: a write outside it shows up as a finite value there
ULP = 2.0 ** -23
N_UNET = 24_417_504     # floats of the flat Unet/resnet34 parameter buffer


def _report(line):
    from conftest import parity_report
    parity_report(line)


def _pair(decoder="unet", C=3, K=2, seed=0):
    from deadtrees_amd.network.unet import UNetHIP
    if decoder == "unet":
        from oracle.unet_ref import make_oracle
        ref = make_oracle(C, K, seed=seed)
    elif decoder == "resunet":
        from oracle.resunet_ref import make_resunet_oracle
        ref = make_resunet_oracle(C, K, seed=seed)
    else:
        from oracle.unetpp_ref import make_unetpp_oracle
        ref = make_unetpp_oracle(C, K, seed=seed)
    m = UNetHIP(in_channels=C, classes=K, decoder=decoder)
    m.load_state_dict(ref.state_dict())
    return ref, m.to(DEV)


def _images(k, B, H, W, C=3, seed=100):
    from deadtrees_amd.data.synthetic import synth_batch
    return [synth_batch(B, H, W, C, 2, seed=seed + i)[0] for i in range(k)]


def _torch_avg(a, p, t, mode, decay):
    """the update as torch tensor expressions (get_swa_multi_avg_fn / get_ema_multi_avg_fn, non-foreach forms)"""
    if t == 0:
        return p.clone()
    return a + (p - a) / (t + 1) if mode == "swa" else a + (p - a) * (1 - decay)


def _assert_avg_close(got, want64, torch32, tag):
    """test 3's bound: relative to max|mean|, at most max(2 x the torch fp32 form's own error, one fp32 ulp)"""
    scale = float(want64.abs().max())
    e_hip = float((got.double() - want64).abs().max()) / scale
    e_torch = float((torch32.double() - want64).abs().max()) / scale
    bound = max(2 * e_torch, ULP)
    _report(f"swa {tag}: err/max|mean| hip {e_hip:.3e} torch-fp32 {e_torch:.3e} bound {bound:.3e} "
            f"ratio {e_hip / bound:.3f}")
    assert e_hip <= bound, (tag, e_hip, e_torch, bound)


# ---------------------------------------------------------------- 3. averaging kernel
@pytest.mark.parametrize("mode,decay", [("swa", 0.0), ("ema", 0.99)])
@pytest.mark.parametrize("n", [1, 3, 4, 1021, N_UNET + 1])
def test_weight_average_kernel(n, mode, decay):
    """40 updates of random-walk parameters against the fp64 running mean / fp64 EMA of the same snapshots."""
    from deadtrees_amd import ops
    g = torch.Generator(device=DEV).manual_seed(n % 1000 + (mode == "ema"))
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    avg = buf[GUARD:GUARD + n]
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    skip = torch.zeros(1, dtype=torch.int32, device=DEV)
    p = torch.randn(n, generator=g, device=DEV)
    a64 = a32 = None
    for t in range(40):
        ops.weight_average(avg, p, count, mode, decay, skip_flag=skip if t % 2 else None)
        a64 = _torch_avg(a64, p.double(), t, mode, decay)
        a32 = _torch_avg(a32, p, t, mode, decay)
        if t == 20:     # a skipped step in the middle: avg and the count stay bit for bit
            before, skip[0] = avg.clone(), 1
            ops.weight_average(avg, p + 1.0, count, mode, decay, skip_flag=skip)
            assert torch.equal(avg, before) and int(count) == t + 1
            skip.zero_()
        p = p + 0.05 * torch.randn(n, generator=g, device=DEV)
    assert int(count) == 40
    assert bool(buf[:GUARD].isnan().all()) and bool(buf[GUARD + n:].isnan().all()), "write outside avg"
    assert not bool(avg.isnan().any())
    _assert_avg_close(avg, a64, a32, f"kernel {mode} n={n}")


def test_weight_averager_object():
    from deadtrees_amd import ops
    p = torch.randn(1000, device=DEV)
    av = ops.WeightAverager(p, ("ema", 0.9))
    assert av.avg.device == p.device and av.avg.dtype == torch.float32 and av.n_averaged == 0
    av.update()
    assert torch.equal(av.avg, p) and av.n_averaged == 1
    p.add_(1.0)
    av.update()
    assert av.n_averaged == 2
    sd = av.state_dict()
    other = ops.WeightAverager(torch.zeros(1000, device=DEV), "swa")
    other.load_state_dict(sd)
    assert other.mode == "ema" and other.decay == 0.9 and other.n_averaged == 2 and torch.equal(other.avg, av.avg)
    tgt = torch.zeros(1000, device=DEV)
    av.copy_to(tgt)
    assert torch.equal(tgt, av.avg)
    with pytest.raises(RuntimeError):
        av.copy_to(torch.zeros(1000))              # a buffer on another device
    with pytest.raises(RuntimeError):
        ops.WeightAverager(torch.zeros(1000), "swa")
    with pytest.raises(ValueError):
        ops.WeightAverager(p, ("ema", 2.0))


# ---------------------------------------------------------------- 4. device-momentum finalize
@pytest.mark.parametrize("P", [1, 64, 256, 300])
@pytest.mark.parametrize("Cc", [16, 64, 512])
def test_bn_finalize_dev_is_bn_finalize(Cc, P):
    """same statistics, same momentum value: every output bit-identical (the two entry points share one kernel);
    P = 300 adds the two-stage reduction.  After k dt_cma_advance calls the momentum read back is 1/k exactly."""
    from deadtrees_amd import ops
    g = torch.Generator().manual_seed(Cc + P)
    stats = torch.rand((2, P, Cc), generator=g) * 50
    stats[1] = stats[1] * stats[1] + 30.0
    stats = stats.to(DEV)
    gamma, beta = (torch.randn(Cc, generator=g).to(DEV) for _ in range(2))
    rm0, rv0 = torch.randn(Cc, generator=g).to(DEV), (torch.rand(Cc, generator=g) + 0.5).to(DEV)
    n_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
    mom = torch.zeros(1, dtype=torch.float32, device=DEV)
    for k in (1, 2, 3, 7):
        while int(n_dev) < k:
            ops.cma_advance(n_dev, mom)
        assert int(n_dev) == k and float(mom) == float(np.float32(1.0 / k))
        rm_a, rv_a, rm_b, rv_b = rm0.clone(), rv0.clone(), rm0.clone(), rv0.clone()
        a = ops.bn_finalize(stats, 64.0 * P, gamma, beta, rm_a, rv_a, momentum=float(np.float32(1.0 / k)))
        b = ops.bn_finalize_dev(stats, 64.0 * P, gamma, beta, rm_b, rv_b, mom)
        for x, y, what in zip(a + (rm_a, rv_a), b + (rm_b, rv_b), ("mean", "invstd", "scale", "shift", "rm", "rv")):
            assert torch.equal(x, y), (what, k)
        assert not torch.equal(rm_a, rm0)


# ---------------------------------------------------------------- 5. update_bn, fp32, against torch on the oracle
def _torch_update_bn64(ref, imgs):
    ref64 = copy.deepcopy(ref).double()
    torch.optim.swa_utils.update_bn([x.double() for x in imgs], ref64)
    return ref64


def _assert_running_stats(m, ref64, tag):
    sd, sd_ref = m.state_dict(), ref64.state_dict()
    worst, worst_k, n = 0.0, None, 0
    for k, v in sd_ref.items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            got, want = sd[k].cpu().double().numpy(), v.numpy()
            r = float(np.max(np.abs(got - want) / (2e-5 + 2e-4 * np.abs(want))))
            if r > worst:
                worst, worst_k = r, k
            n += 1
    _report(f"update_bn {tag}: {n} tensors, worst |d| / (2e-5 + 2e-4 |ref|) = {worst:.3f} ({worst_k})")
    for k, v in sd_ref.items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            np.testing.assert_allclose(sd[k].cpu().numpy(), v.numpy(), rtol=2e-4, atol=2e-5, err_msg=k)
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(v), k


@pytest.mark.parametrize("k,B,S", [(5, 4, 64), (3, 2, 256)])
def test_update_bn_fp32_against_torch_on_fp64_oracle(k, B, S):
    ref, m = _pair()
    imgs = _images(k, B, S, S)
    ref64 = _torch_update_bn64(ref, imgs)
    # a training forward first: the running statistics and counters are NOT at their reset values when update_bn starts
    m.train()
    with torch.no_grad():
        m(imgs[0].to(DEV))
    before = m.flat_params.detach().clone()
    assert m.update_bn([x.to(DEV) for x in imgs]) == k
    assert torch.equal(m.flat_params.detach(), before)
    _assert_running_stats(m, ref64, f"fp32 {k}x{B}x3x{S}x{S}")
    assert int(m.num_batches_tracked.min()) == int(m.num_batches_tracked.max()) == k


def test_update_bn_contract_flags_batch_forms_and_empty_input():
    ref, m = _pair()
    imgs = [x.to(DEV) for x in _images(2, 2, 64, 64)]
    want = None
    forms = [imgs, [(x, None) for x in imgs], [[x, 0] for x in imgs]]
    for (tr, enc_tr), batches in zip([(True, True), (True, False), (False, True), (False, False)], forms + forms[:1]):
        m.train(tr)
        m.encoder.train(enc_tr)
        m.update_bn(batches)
        assert m.training is tr and m.encoder.training is enc_tr
        want = m.bn_state.clone() if want is None else want
        assert torch.equal(m.bn_state, want)          # the flags change nothing: every BatchNorm uses batch statistics
    # the datamodule's dict batches, image moved by to_device
    mask = torch.zeros((2, 64, 64), dtype=torch.int64)
    m.update_bn([{"main": (x.cpu(), mask, None, None, None)} for x in imgs], to_device=DEV)
    assert torch.equal(m.bn_state, want)
    state, nbt, params = m.bn_state.clone(), m.num_batches_tracked.clone(), m.flat_params.detach().clone()
    with pytest.raises(ValueError):
        m.update_bn([])
    with pytest.raises(ValueError):
        m.update_bn(iter(()))
    assert torch.equal(m.bn_state, state) and torch.equal(m.num_batches_tracked, nbt)
    assert torch.equal(m.flat_params.detach(), params)
    with pytest.raises(TypeError):
        m.update_bn([42])
    with pytest.raises(RuntimeError):
        m.update_bn([imgs[0].cpu()])


@pytest.mark.parametrize("decoder", ["resunet", "unetplusplus"])
def test_update_bn_other_decoders_against_their_oracles(decoder):
    ref, m = _pair(decoder)
    imgs = _images(3, 2, 64, 64)
    ref64 = _torch_update_bn64(ref, imgs)
    before = m.flat_params.detach().clone()
    m.update_bn([x.to(DEV) for x in imgs])
    assert torch.equal(m.flat_params.detach(), before)
    _assert_running_stats(m, ref64, f"fp32 {decoder}")


# ---------------------------------------------------------------- 6. update_bn, bf16
def _bn_tensors(m, state):
    """{name: tensor} views of a bn_state-shaped tensor"""
    out = {}
    for c in m.spec.convs:
        if c.bn_key is not None:
            out[c.bn_key + ".running_mean"] = state[2 * c.bn_off:2 * c.bn_off + c.cout]
            out[c.bn_key + ".running_var"] = state[2 * c.bn_off + c.cout:2 * c.bn_off + 2 * c.cout]
    return out


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_update_bn_k_batches_is_the_mean_of_one_batch_results(precision):
    """(i) the k-batch result equals the fp64 mean of the k one-batch results of the same kernels within
    k * 2^-23 * max(|tensor|, 1): all that the fp32 cumulative average can lose"""
    _, m = _pair()
    k = 4
    imgs = [x.to(DEV) for x in _images(k, 2, 64, 64)]
    singles = []
    for x in imgs:
        m.update_bn([x], precision=precision)
        singles.append(m.bn_state.double().clone())
    mean64 = torch.stack(singles).mean(0)
    m.update_bn(imgs, precision=precision)
    assert bool(torch.isfinite(m.bn_state).all())
    worst = 0.0
    got, want = _bn_tensors(m, m.bn_state.double()), _bn_tensors(m, mean64)
    for name in want:
        bound = k * ULP * max(float(want[name].abs().max()), 1.0)
        err = float((got[name] - want[name]).abs().max())
        worst = max(worst, err / bound)
        assert err <= bound, (name, err, bound)
    _report(f"update_bn {precision} consistency, k={k}: worst err / (k 2^-23 max(|t|,1)) = {worst:.3f}")


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_update_bn_one_batch_is_the_training_steps_batch_statistics(precision):
    """(ii) one batch: the momentum is 1 and the running statistics ARE the batch statistics.  The existing training step
    leaves r1 = (1 - 0.1f) r0 + 0.1f b for the same weights and batch with r0 = 0 / 1: b solved from it in fp64 must agree
    within 2^-19 max(|tensor|, 1) — the rounding of r1 amplified tenfold, nothing else, because the recalibration
    forward runs the same kernels on the same data.
    Measured on an MI355X: see DESIGN §12."""
    from deadtrees_amd.data.synthetic import synth_batch
    from deadtrees_amd.trainer import HipTrainer
    _, m = _pair()
    img, mask = (t.to(DEV) for t in synth_batch(2, 64, 64, 3, 2, seed=5))
    m.update_bn([img], precision=precision)
    recal = m.bn_state.double().clone()
    _, m2 = _pair()
    r0 = m2.bn_state.double().clone()
    HipTrainer(m2, precision=precision).step(img, mask)
    mom = float(np.float32(0.1))
    keep = float(np.float32(1.0) - np.float32(0.1))
    b = (m2.bn_state.double() - keep * r0) / mom
    worst = 0.0
    got, want = _bn_tensors(m, recal), _bn_tensors(m, b)
    for name in want:
        bound = 2.0 ** -19 * max(float(want[name].abs().max()), 1.0)
        err = float((got[name] - want[name]).abs().max())
        worst = max(worst, err / bound)
        assert err <= bound, (name, err, bound)
    _report(f"update_bn {precision} one batch vs training step: worst err / (2^-19 max(|t|,1)) = {worst:.3f}")


# ---------------------------------------------------------------- 7. replay
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_update_bn_graph_replay_equals_eager(precision):
    """two eager batches, capture, two replays: the momentum changes every batch and travels on the device"""
    from deadtrees_amd.trainer import HipTrainer
    _, m = _pair()
    imgs = [x.to(DEV) for x in _images(4, 2, 64, 64)]
    eager = HipTrainer(m, precision=precision)
    assert eager.update_bn(imgs) == 4
    want = m.bn_state.clone()
    tr = HipTrainer(m, precision=precision, graph=True)
    assert tr.update_bn(imgs) == 4
    assert len(tr._recal_replays) == 1 and tr._recal_replays.values()[0].captured
    assert torch.equal(m.bn_state, want)
    assert tr.update_bn(imgs + imgs[:1]) == 5          # a second pass replays the same graph from batch one
    got5 = m.bn_state.clone()
    eager.update_bn(imgs + imgs[:1])
    assert torch.equal(m.bn_state, got5)
    assert int(m.num_batches_tracked.max()) == 5


# ---------------------------------------------------------------- 8. launch trimming
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_recalibration_forward_launches_no_head_and_no_last_normalise(precision):
    _, m = _pair()
    x = _images(1, 2, 64, 64)[0].to(DEV)
    m.update_bn([x], precision=precision)
    rec = m.engine.recal_launches
    kinds = [k for k, _ in rec]
    bn_convs = [c for c in m.spec.convs if c.bn_key is not None]
    last = m.spec.decoder[-1].conv2
    assert "head" not in kinds
    assert ("bn_act", last.key) not in rec
    assert rec[-1] == ("bn_finalize_dev", last.key)
    assert sorted(key for k, key in rec if k == "bn_finalize_dev") == sorted(c.key for c in bn_convs)
    assert kinds.count("conv") == len(bn_convs)
    assert any(k == "bn_act" for k in kinds)
    assert m.engine.saved is None                      # nothing kept for a backward
    # the training-statistics forward the parent offers for this launches both
    m.train()
    with torch.no_grad():
        m(x)
    assert m.engine.recal_launches is rec              # an ordinary forward records nothing


# ---------------------------------------------------------------- 9. EMA inside the step
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_ema_inside_the_step(precision):
    from deadtrees_amd.data.synthetic import synth_batch
    from deadtrees_amd.trainer import HipTrainer
    decay = 0.99
    batches = [tuple(t.to(DEV) for t in synth_batch(2, 64, 64, 3, 2, seed=s)) for s in range(3)]
    out = {}
    for mode in ("eager", "graph", "none"):
        _, m = _pair()
        tr = HipTrainer(m, precision=precision, graph=(mode == "graph"), average=None if mode == "none" else ("ema", decay))
        assert (tr.averager is None) == (mode == "none")
        losses, snaps = [], []
        for s in range(6):
            losses.append(float(tr.step(*batches[s % 3])))
            if mode == "eager":
                snaps.append(m.flat_params.detach().clone())
        out[mode] = (losses, m.flat_params.detach().clone(), m.bn_state.clone(),
                     None if tr.averager is None else tr.averager.avg.clone(),
                     None if tr.averager is None else tr.averager.n_averaged, snaps)
        if mode == "graph":
            assert tr._step_replays.values()[0].captured
        if mode == "eager":     # a non-finite loss: the step is skipped, avg and its count stay
            bad = batches[0][0].clone()
            bad[0, 0, 0, 0] = float("nan")
            before = tr.averager.avg.clone()
            tr.step(bad, batches[0][1])
            assert int(tr.last["skipped"]) == 1
            assert torch.equal(tr.averager.avg, before) and tr.averager.n_averaged == 6
            tr.step(*batches[1])
            assert tr.averager.n_averaged == 7 and not torch.equal(tr.averager.avg, before)
    le, pe, be, ae, ne, snaps = out["eager"]
    lg, pg, bg, ag, ng, _ = out["graph"]
    ln, pn, bn, _, _, _ = out["none"]
    assert ne == ng == 6
    assert torch.equal(ae, ag)
    assert le == lg == ln
    assert torch.equal(pe, pn) and torch.equal(be, bn) and torch.equal(pe, pg) and torch.equal(be, bg)
    a64 = a32 = None
    for t, p in enumerate(snaps):
        a64 = _torch_avg(a64, p.double(), t, "ema", decay)
        a32 = _torch_avg(a32, p, t, "ema", decay)
    _assert_avg_close(ae, a64, a32, f"EMA in the {precision} step")


# ---------------------------------------------------------------- 10. end to end
def _torch_lr_sequence(epochs, base_lr, t_max, cfg):
    from torch.optim.lr_scheduler import CosineAnnealingLR
    from torch.optim.swa_utils import SWALR
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=base_lr)
    sched, lrs = CosineAnnealingLR(opt, T_max=t_max), []
    for e in range(epochs):
        if e == cfg.swa_start:      # SWA takes over from the rate the cosine schedule had reached
            sched = SWALR(opt, swa_lr=cfg.swa_lr, anneal_epochs=cfg.anneal_epochs, anneal_strategy=cfg.anneal_strategy)
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    return lrs


def _swa_loader():
    from deadtrees_amd.data.synthetic import synth_batch
    return [synth_batch(2, 64, 64, 3, 2, seed=40 + i) + (None, None, None) for i in range(2)]


def test_fit_with_swa_end_to_end_fp32(tmp_path):
    from deadtrees_amd.trainer import HipTrainer, SWAConfig, fit
    ref, m = _pair()
    tr = HipTrainer(m, average="swa")
    cfg = SWAConfig(swa_start=2, swa_lr=1e-4, anneal_epochs=2)
    loader = _swa_loader()
    snaps = []
    hist = fit(tr, loader, epochs=5, base_lr=3e-4, t_max=10, to_device=DEV, swa=cfg,
               on_epoch_end=lambda rec: snaps.append(m.flat_params.detach().clone()))
    assert hist[-1] == {"swa/bn_batches": 2}
    assert [h["swa/n_averaged"] for h in hist[:-1]] == [0, 0, 1, 2, 3]
    want_lr = _torch_lr_sequence(5, 3e-4, 10, cfg)
    for h, w in zip(hist[:-1], want_lr):
        assert h["lr"] == pytest.approx(w, rel=1e-12, abs=0.0), (h, want_lr)
    # the average, teacher-forced on the HIP trajectory: fp64 mean of the parameters at the end of epochs 2-4
    a64 = a32 = None
    for t, p in enumerate(snaps[2:]):
        a64 = _torch_avg(a64, p.double(), t, "swa", 0.0)
        a32 = _torch_avg(a32, p, t, "swa", 0.0)
    assert float((a64 - torch.stack([p.double() for p in snaps[2:]]).mean(0)).abs().max()) < 1e-12
    _assert_avg_close(tr.averager.avg, a64, a32, "fit, epochs 2-4")
    assert torch.equal(m.flat_params.detach(), tr.averager.avg)
    # running statistics: torch's update_bn on the fp64 oracle loaded with the averaged weights
    ref64 = copy.deepcopy(ref).double()
    ref64.load_state_dict(m.state_dict())
    torch.optim.swa_utils.update_bn([b[0].double() for b in loader], ref64)
    _assert_running_stats(m, ref64, "after fit(swa)")
    m.eval()
    ref64.eval()
    x = loader[0][0]
    with torch.no_grad():
        want = ref64(x.double())
        got = m(x.to(DEV)).cpu().double()
    err, scale = float((got - want).abs().max()), float(want.abs().max())
    _report(f"fit(swa) final eval logits: err {err / scale:.3e} of max|logit| (bound 1e-4)")
    assert err <= 1e-4 * scale, (err, scale)
    # the result is an ordinary model: its state_dict round-trips through load_state_dict and the restricted .ckpt reader
    from deadtrees_amd.network.unet import UNetHIP
    from deadtrees_amd.utils.ckpt import lightning_state_dict
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    path = tmp_path / "swa.ckpt"
    torch.save({"state_dict": {f"model.{k}": v for k, v in sd.items()}}, str(path))
    for loaded in (sd, lightning_state_dict(path)):
        m2 = UNetHIP()
        m2.load_state_dict(loaded)
        assert torch.equal(m2.flat_params.detach(), m.flat_params.detach().cpu())
        assert torch.equal(m2.bn_state, m.bn_state.cpu())
        sd2 = m2.state_dict()
        assert set(sd2) == set(sd)
        for k in sd:
            assert torch.equal(sd2[k], sd[k]), k
            if k.endswith("num_batches_tracked"):
                assert int(sd2[k]) == 2, k


def test_fit_with_swa_bf16_graph_completes():
    from deadtrees_amd.trainer import HipTrainer, SWAConfig, fit
    _, m = _pair()
    tr = HipTrainer(m, precision="bf16", graph=True, average="swa")
    hist = fit(tr, _swa_loader(), epochs=5, to_device=DEV, swa=SWAConfig(swa_start=2, anneal_epochs=2))
    assert hist[-1] == {"swa/bn_batches": 2} and hist[-2]["swa/n_averaged"] == 3
    assert bool(torch.isfinite(m.bn_state).all()) and bool(torch.isfinite(m.flat_params).all())
    assert torch.equal(m.flat_params.detach(), tr.averager.avg)
    assert all(math.isfinite(h["train/total_loss"]) for h in hist[:-1])


def test_no_average_allocates_nothing():
    from deadtrees_amd.trainer import HipTrainer
    _, m = _pair()
    tr = HipTrainer(m)
    assert tr.averager is None
    for call in (tr.update_average, tr.swap_in_average):
        with pytest.raises(RuntimeError):
            call()


def test_fit_with_swa_and_multistage_callback():
    """the callback's stages run as before (encoder in eval mode, a fresh Adam and cosine schedule at lr_reduce_epoch);
    SWA takes over at swa_start from the rate THAT schedule had reached; the final recalibration covers the encoder's
    BatchNorm layers although the encoder view is in eval mode, and leaves it there"""
    from torch.optim.swa_utils import SWALR
    from deadtrees_amd.callbacks.multistage import MultiStage
    from deadtrees_amd.network.segmodel import cosine_lr
    from deadtrees_amd.trainer import HipTrainer, SWAConfig, fit
    _, m = _pair()
    m.encoder_weights = "given"          # (the callback only asks whether there are any)
    tr = HipTrainer(m, average="swa")
    enc_stats = m.bn_state[:2 * 64].clone()
    cb = MultiStage(unfreeze_epoch=100, lr_reduce_epoch=2, lr_reduce_fraction=3)
    hist = fit(tr, _swa_loader(), epochs=6, base_lr=3e-4, t_max=10, to_device=DEV, callbacks=[cb],
               swa=SWAConfig(swa_start=4, swa_lr=5e-5, anneal_epochs=2))
    want = [cosine_lr(3e-4, 0, 10), cosine_lr(3e-4, 1, 10), cosine_lr(1e-4, 0, 10), cosine_lr(1e-4, 1, 10)]
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=cosine_lr(1e-4, 2, 10))
    sched = SWALR(opt, swa_lr=5e-5, anneal_epochs=2)
    for _ in range(2):
        want.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    for h, w in zip(hist[:-1], want):
        assert h["lr"] == pytest.approx(w, rel=1e-12, abs=0.0), (h, want)
    assert [h["swa/n_averaged"] for h in hist[:-1]] == [0, 0, 0, 0, 1, 2] and hist[-1] == {"swa/bn_batches": 2}
    assert m.training and not m.encoder.training
    assert torch.equal(m.flat_params.detach(), tr.averager.avg)
    assert int(m.num_batches_tracked[0]) == 2
    assert not torch.equal(m.bn_state[:2 * 64], enc_stats) and bool(torch.isfinite(m.bn_state).all())
