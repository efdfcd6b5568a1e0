"""Pretrained encoder surface without a GPU: ``encoder_weights=``, the ``model.encoder`` view, smp's decoder init,
and the ``MultiStage`` callback driven through ``fit(callbacks=)``."""
import socket

import pytest
import torch

IMAGENET_FILE = "resnet34-333f7ec4.pth"


def UNetHIP(**kw):
    from deadtrees_amd.network.unet import UNetHIP as U
    return U(**kw)


def _torchvision_resnet34(seed=0):
    """a synthetic state_dict in torchvision's resnet34 layout (fc included)"""
    g = torch.Generator().manual_seed(seed)
    m = UNetHIP(in_channels=3)
    sd = {}
    for k, v in m.smp_state_dict().items():
        if k.startswith("encoder."):
            sd[k[len("encoder."):]] = torch.randn(v.shape, generator=g) if v.is_floating_point() else v.clone()
    sd["fc.weight"] = torch.randn(1000, 512, generator=g)
    sd["fc.bias"] = torch.randn(1000, generator=g)
    return sd


@pytest.fixture
def no_network(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("network access attempted")
    monkeypatch.setattr(socket.socket, "connect", refuse)
    monkeypatch.setattr(socket, "create_connection", refuse)


def test_imagenet_from_hub_cache_and_path(tmp_path, monkeypatch, no_network):
    monkeypatch.setenv("TORCH_HOME", str(tmp_path))
    sd = _torchvision_resnet34()
    (tmp_path / "hub" / "checkpoints").mkdir(parents=True)
    path = tmp_path / "hub" / "checkpoints" / IMAGENET_FILE
    torch.save(sd, path)
    for w in ("imagenet", str(path)):
        m = UNetHIP(encoder_weights=w)
        assert m.encoder_weights == w
        enc = m.encoder.state_dict()
        assert not [k for k in enc if k.startswith("fc.")]
        for k, v in sd.items():
            if not k.startswith("fc."):
                assert torch.equal(enc[k], v), k


@pytest.mark.parametrize("cin", [1, 3, 4])
def test_first_conv_patch(tmp_path, cin):
    from deadtrees_amd.network.unet import patch_first_conv
    sd = _torchvision_resnet34()
    p = tmp_path / "enc.pth"
    torch.save(sd, p)
    m = UNetHIP(in_channels=cin, encoder_weights=str(p))
    w = m.encoder.state_dict()["conv1.weight"]
    w3 = sd["conv1.weight"]
    assert w.shape == (64, cin, 7, 7)
    if cin == 1:
        expect = w3.sum(1, keepdim=True)
    elif cin == 3:
        expect = w3
    else:
        expect = torch.stack([w3[:, i % 3] for i in range(cin)], 1) * (3 / cin)
    assert torch.allclose(w, expect, rtol=0, atol=1e-6)
    assert torch.equal(patch_first_conv(w3, 3), w3)


def test_errors(tmp_path, monkeypatch, no_network):
    monkeypatch.setenv("TORCH_HOME", str(tmp_path))
    with pytest.raises(FileNotFoundError, match=str(tmp_path / "hub" / "checkpoints" / IMAGENET_FILE)):
        UNetHIP(encoder_weights="imagenet")
    with pytest.raises(FileNotFoundError, match="nowhere.pth"):
        UNetHIP(encoder_weights=str(tmp_path / "nowhere.pth"))
    sd = _torchvision_resnet34()
    del sd["layer2.1.bn2.running_var"]
    torch.save(sd, tmp_path / "missing.pth")
    with pytest.raises(RuntimeError, match="layer2.1.bn2.running_var"):
        UNetHIP(encoder_weights=str(tmp_path / "missing.pth"))
    sd = _torchvision_resnet34()
    sd["layer3.0.conv1.weight"] = torch.zeros(256, 128, 3, 1)
    torch.save(sd, tmp_path / "shape.pth")
    with pytest.raises(RuntimeError, match="size mismatch"):
        UNetHIP(encoder_weights=str(tmp_path / "shape.pth"))


def test_decoder_init_is_smp(tmp_path):
    torch.save(_torchvision_resnet34(), tmp_path / "enc.pth")
    with torch.random.fork_rng():       # the init draws from torch's global generator: leave it as it was
        torch.manual_seed(0)
        m = UNetHIP(in_channels=4, classes=2, encoder_weights=str(tmp_path / "enc.pth"))
    sd = m.smp_state_dict()
    for c in m.spec.convs:
        if c.key.startswith("encoder."):
            continue
        w = sd[c.key]
        fan_in = c.cin * c.state_k ** 2
        if c is m.spec.head:
            expect = (2.0 / (fan_in + c.cout * c.state_k ** 2)) ** 0.5       # xavier_uniform_
            assert float(sd[c.key.replace(".weight", ".bias")].abs().max()) == 0.0
        else:
            expect = (2.0 / fan_in) ** 0.5                                   # kaiming_uniform_(fan_in, relu)
            assert torch.equal(sd[f"{c.bn_key}.weight"], torch.ones(c.cout))
            assert torch.equal(sd[f"{c.bn_key}.bias"], torch.zeros(c.cout))
        assert float(w.std()) == pytest.approx(expect, rel=0.1 if w.numel() > 1000 else 0.35), c.key


def test_encoder_view_surface(tmp_path):
    m = UNetHIP(in_channels=4)
    keys0 = sorted(m.state_dict())
    n0 = sum(p.numel() for p in m.parameters())
    assert list(m.encoder.parameters()) == []
    enc = m.encoder.state_dict()
    assert "conv1.weight" in enc and "layer4.2.bn2.running_var" in enc and "bn1.num_batches_tracked" in enc
    assert len(enc) == len([k for k in keys0 if k.startswith("encoder.")])
    m2 = UNetHIP(in_channels=4)
    m2.encoder.load_state_dict(enc)
    for k, v in m2.encoder.state_dict().items():
        assert torch.equal(v, enc[k]), k
    assert sorted(m.state_dict()) == keys0
    assert sum(p.numel() for p in m.parameters()) == n0
    # modes: the owner's train()/eval() recurse; the encoder's own mode is independent
    m.train()
    m.encoder.eval()
    assert m.training and not m.encoder.training and not m._encoder_training()
    m.eval()
    m.train()
    assert m.encoder.training
    # the reference's loop: an attribute assignment, a no-op
    for mod in m.encoder.modules():
        mod.requires_grad_ = False
    assert not m.encoder_frozen and m.trainable_ranges() is None
    m.encoder.requires_grad_(False)
    assert m.encoder_frozen and m.trainable_ranges() == [(m.encoder_hi, m.spec.n_params)]
    assert m.encoder_hi == min(c.w_off for c in m.spec.convs if not c.key.startswith("encoder."))


def test_semsegment_passes_encoder_weights(tmp_path):
    from deadtrees_amd.network.segmodel import SemSegment
    from deadtrees_amd.utils.config import default_network, default_training
    torch.save(_torchvision_resnet34(), tmp_path / "enc.pth")
    net = default_network()
    net["encoder_weights"] = str(tmp_path / "enc.pth")
    s = SemSegment(net, default_training())
    assert s.encoder_weights == str(tmp_path / "enc.pth")
    assert s.model.encoder_weights == str(tmp_path / "enc.pth")


class _StubOpt:
    def __init__(self):
        self.lr, self.resets = 3e-4, []

    def reset_state(self, lr=None):
        self.resets.append(lr)
        self.lr = lr

    def set_trainable(self, ranges):
        pass


class _StubTrainer:
    """HipTrainer's interface to fit() with CPU-only state: records the encoder mode and lr of every step"""

    def __init__(self, model):
        self.model, self.opt, self.log = model, _StubOpt(), []

    def step(self, img, mask, distmap=None, alpha=1.0):   # noqa: ARG002
        self.log.append((self.model.encoder.training, self.model.encoder_frozen, self.opt.lr))
        return torch.zeros(())


@pytest.mark.parametrize("freeze_weights", [False, True])
def test_multistage_through_fit(tmp_path, freeze_weights):
    from deadtrees.callbacks.multistage import MultiStage
    from deadtrees_amd.network.segmodel import cosine_lr
    from deadtrees_amd.trainer import fit
    torch.save(_torchvision_resnet34(), tmp_path / "enc.pth")
    m = UNetHIP(encoder_weights=str(tmp_path / "enc.pth"))
    tr = _StubTrainer(m)
    loader = [(torch.zeros(1), torch.zeros(1), None, None, None)]
    cb = MultiStage(unfreeze_epoch=20, lr_reduce_epoch=40, lr_reduce_fraction=3, freeze_weights=freeze_weights)
    fit(tr, loader, epochs=45, base_lr=3e-4, t_max=10, callbacks=[cb])
    enc_train = [e[0] for e in tr.log]
    frozen = [e[1] for e in tr.log]
    assert enc_train[:20] == [False] * 20 and enc_train[20:] == [True] * 25
    assert frozen == ([True] * 20 + [False] * 25 if freeze_weights else [False] * 45)
    assert tr.opt.resets == [pytest.approx(1e-4)]
    lrs = [e[2] for e in tr.log]
    assert lrs[39] == pytest.approx(cosine_lr(3e-4, 39, 10))
    for ep in range(40, 45):
        assert lrs[ep] == pytest.approx(cosine_lr(1e-4, ep - 40, 10)), ep


def test_multistage_exits_without_weights():
    from deadtrees_amd.callbacks.multistage import MultiStage
    from deadtrees_amd.trainer import fit
    m = UNetHIP()
    tr = _StubTrainer(m)
    with pytest.raises(SystemExit):
        fit(tr, [(torch.zeros(1), torch.zeros(1), None, None, None)], epochs=1, callbacks=[MultiStage(unfreeze_epoch=2)])
    assert tr.log == []
