"""architecture "efficientunet++" (reference segmodel.py:68-71) — host side: the torch restatement tests/effunetpp_ref.py
against the fixtures written by executing the reference's decoder (tests/make_golden_effunetpp.py), the flat parameter
buffer's new tensor kinds (conv bias in front of BatchNorm, depthwise weights, cSE / sSE layers), the inference-only door
of ``SemSegment`` and the refusals of every training entry point.  No GPU needed."""
import os

import pytest
import torch

from effunetpp_ref import EfficientUnetPlusPlusDecoderRef, make_effunetpp_oracle

N_PARAMS_S1E1 = 26_963_016     # encoder 21,284,672 + EfficientUnet++ decoder (squeeze 1, expansion 1) + 3x3 head, K = 2, C = 3
N_PARAMS_S2E2 = 32_220_184


def _model(**kw):
    from deadtrees_amd.network.unet import UNetHIP
    return UNetHIP(decoder="efficientunetplusplus", **kw)


@pytest.mark.parametrize("squeeze,expansion", [(1, 1), (2, 2)])
def test_restatement_matches_the_executed_reference_decoder(golden_dir, squeeze, expansion):
    from oracle.golden import load_npz_parts
    z = load_npz_parts(os.path.join(golden_dir, f"effunetpp_decoder_s{squeeze}e{expansion}"))
    assert tuple(z["ratios"]) == (squeeze, expansion)
    dec = EfficientUnetPlusPlusDecoderRef(tuple(z["enc_ch"]), tuple(z["dec_ch"]), squeeze, expansion).eval()
    sd = {k[3:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("sd:")}
    mine = dec.state_dict()
    assert list(mine) == list(sd)                                   # names AND order of the reference's state_dict
    for k, v in mine.items():
        assert tuple(v.shape) == tuple(sd[k].shape), k
    dec.load_state_dict(sd)
    C0 = int(z["enc_ch"][0])
    feats = [torch.zeros(2, C0, 32, 32)] + [torch.from_numpy(z[f"feat{i}"]) for i in range(1, 6)]
    with torch.no_grad():
        out = dec(*feats)
    want = torch.from_numpy(z["out"])
    err = float((out - want).abs().max())
    print(f"effunet++ restatement s{squeeze}e{expansion}: max|err| {err:.3e}, max|out| {float(want.abs().max()):.3e}")
    assert err <= 1e-5 * float(want.abs().max())


@pytest.mark.parametrize("squeeze,expansion,n", [(1, 1, N_PARAMS_S1E1), (2, 2, N_PARAMS_S2E2)])
def test_state_dict_keys_and_parameter_count_equal_the_oracle(squeeze, expansion, n):
    ref = make_effunetpp_oracle(3, 2, seed=1, squeeze=squeeze, expansion=expansion)
    m = _model(squeeze_ratio=squeeze, expansion_ratio=expansion)
    sd, rsd = m.state_dict(), ref.state_dict()
    assert set(sd) == set(rsd)
    for k, v in rsd.items():
        assert tuple(sd[k].shape) == tuple(v.shape), k
    assert m.spec.n_true_params == sum(p.numel() for p in ref.parameters()) == n
    blk = m.spec.decoder[0].conv1
    assert (blk.cin, blk.mid, blk.cout, blk.cse1.cout) == (768, 768 * expansion, 256, 768 * expansion // squeeze)
    assert m.spec.decoder[-1].conv2.mid == 16 * expansion and m.spec.decoder[-1].conv2.skip is None
    assert all(d.conv1.skip is not None for d in m.spec.decoder)


def test_load_and_save_round_trip_exactly():
    ref = make_effunetpp_oracle(4, 3, seed=2, squeeze=2, expansion=2)
    m = _model(in_channels=4, classes=3, squeeze_ratio=2, expansion_ratio=2)
    m.load_state_dict(ref.state_dict())
    for out in (m.state_dict(), m.smp_state_dict()):
        for k, v in ref.state_dict().items():
            assert torch.equal(out[k], v), k
    m2 = _model(in_channels=4, classes=3, squeeze_ratio=2, expansion_ratio=2)
    m2.load_smp_state_dict(m.smp_state_dict())
    assert torch.equal(m2.flat_params, m.flat_params) and torch.equal(m2.bn_state, m.bn_state)
    with pytest.raises(RuntimeError, match="size mismatch"):
        _model(in_channels=4, classes=3).load_smp_state_dict(m.smp_state_dict())


def test_reset_parameters_zeroes_every_bias_and_draws_kaiming_weights():
    ref = make_effunetpp_oracle(3, 2, seed=3)
    m = _model()
    m.load_state_dict(ref.state_dict())
    m.reset_parameters(seed=5)
    sd = m.state_dict()
    bn = {k[:-len(".running_mean")] for k in sd if k.endswith(".running_mean")}
    n_bias = 0
    for k, v in sd.items():
        if k.endswith(".bias"):
            assert not v.any(), k
            n_bias += k[:-len(".bias")] not in bn
        elif k.endswith(".weight") and k[:-len(".weight")] in bn:
            assert torch.equal(v, torch.ones_like(v)), k
    assert n_bias == 1 + 11 * (2 * 6 + 1)       # head + per node: 6 biased convolutions per block, one skip projection
    w = sd["decoder.blocks.x_0_0.conv1.block.3.weight"]                # depthwise [768,1,3,3]: fan_in 9
    assert tuple(w.shape) == (768, 1, 3, 3) and abs(float(w.std()) - (2.0 / 9) ** 0.5) < 0.02
    w = sd["decoder.blocks.x_0_0.conv1.block.0.weight"]                # 1x1 [768,768,1,1]: fan_in 768
    assert abs(float(w.std()) - (2.0 / 768) ** 0.5) < 0.002


def test_semsegment_inference_only_door():
    from deadtrees.network.segmodel import SemSegment
    from deadtrees_amd.utils.config import default_network, default_training
    for arch in ("efficientunet++", "EfficientUnetPlusPlus"):
        with pytest.raises(NotImplementedError):
            SemSegment(default_network(architecture=arch), default_training())
        m = SemSegment(default_network(architecture=arch), default_training(), inference_only=True)
        assert m.model.spec.decoder_kind == "efficientunetplusplus" and m.inference_only
        assert not m.training and not m.model.training
        for hook in (m.train, lambda: m.training_step(None, 0), m.configure_optimizers):
            with pytest.raises(NotImplementedError):
                hook()
        assert m.eval() is m
    m = SemSegment(default_network(architecture="efficientunet++", squeeze_ratio=4, expansion_ratio=2), default_training(),
                   inference_only=True)
    assert (m.model.spec.squeeze_ratio, m.model.spec.expansion_ratio) == (4, 2)
    for arch in ("resunet++", "resunetplusplus"):
        for kw in ({}, {"inference_only": True}):
            with pytest.raises(NotImplementedError):
                SemSegment(default_network(architecture=arch), default_training(), **kw)
    with pytest.raises(NotImplementedError):
        SemSegment(default_network(architecture="efficientunet++", encoder_name="efficientnet-b5"), default_training(),
                   inference_only=True)
    assert SemSegment(default_network(), default_training(), inference_only=True).training is False


def test_checkpoint_written_by_the_projects_writer_loads_with_ratios_from_shapes(tmp_path):
    import json
    from deadtrees.network.segmodel import SemSegment
    from deadtrees_amd.trainer import checkpoint_writer
    from deadtrees_amd.utils.ckpt import infer_network_conf
    ref = make_effunetpp_oracle(4, 3, seed=4, squeeze=2, expansion=2)
    m = _model(in_channels=4, classes=3, squeeze_ratio=2, expansion_ratio=2)
    m.load_state_dict(ref.state_dict())
    path = tmp_path / "eff.ckpt"
    checkpoint_writer(m)(str(path))
    got = SemSegment.load_from_checkpoint(str(path))
    assert got.inference_only and not got.training
    assert (got.model.spec.squeeze_ratio, got.model.spec.expansion_ratio) == (2, 2)
    assert (got.in_channels, len(got.classes)) == (4, 3)
    for k, v in ref.state_dict().items():
        assert torch.equal(got.model.state_dict()[k], v), k
    # the ratios come from the tensor shapes: a file whose recorded hyper-parameters lack (or contradict) them loads alike
    ck = torch.load(str(path), weights_only=True)
    hp = json.loads(ck["hyper_parameters_json"])
    hp["network"].update(squeeze_ratio=1, expansion_ratio=1)
    ck["hyper_parameters_json"] = json.dumps(hp)
    torch.save(ck, str(tmp_path / "lying.ckpt"))
    got = SemSegment.load_from_checkpoint(str(tmp_path / "lying.ckpt"))
    assert (got.model.spec.squeeze_ratio, got.model.spec.expansion_ratio) == (2, 2)
    net = infer_network_conf(ref.state_dict())
    assert (net["architecture"], net["squeeze_ratio"], net["expansion_ratio"]) == ("efficientunet++", 2, 2)
    assert infer_network_conf(_unet_sd())["architecture"] == "unet"


def _unet_sd():
    from deadtrees_amd.network.unet import UNetHIP
    return UNetHIP().state_dict()


def test_training_entry_points_raise_before_anything_runs():
    from deadtrees_amd.trainer import HipTrainer
    m = _model()
    x = torch.zeros(1, 3, 32, 32)
    m.train()
    with pytest.raises(NotImplementedError, match="backward"):
        m(x)
    m.eval()
    with pytest.raises(NotImplementedError, match="bf16"):
        m.predict_logits(x, precision="bf16")
    with pytest.raises(NotImplementedError, match="bf16"):
        m.predict_classes(x, precision="bf16")
    with pytest.raises(NotImplementedError, match="bf16"):
        m.precision = "bf16"
    assert m.precision == "fp32"
    with pytest.raises(NotImplementedError, match="backward"):
        HipTrainer(m)
    assert m.deliver_grad_to_autograd is True       # the refused trainer left the model untouched
    before = m.bn_state.clone()
    with pytest.raises(NotImplementedError, match="update_bn"):
        m.update_bn([x])
    assert torch.equal(m.bn_state, before)
    from deadtrees_amd.network.spec import build_spec
    with pytest.raises(ValueError):
        build_spec(decoder="unet", squeeze_ratio=2)
    with pytest.raises(ValueError):
        build_spec(decoder="efficientunetplusplus", squeeze_ratio=3)


def test_new_kernels_validate_shapes_on_the_host():
    """shape preconditions of csrc/mbconv.hip are refused through dt_last_error before any launch (no GPU needed)"""
    from deadtrees_amd import _lib
    lib = _lib.load()
    p = 4096      # never dereferenced: every call below fails validation first
    assert lib.dt_pwconv_affine(p, None, p, p, p, p, None, None, None, 1, 4, 4, 24, 0, 0, 16, 0, None) < 0
    assert b"multiples of 16" in lib.dt_last_error()
    assert lib.dt_pwconv_affine(p, None, p, p, p, p, p, None, None, 1, 4, 4, 16, 0, 0, 16, 0, None) < 0
    assert b"gate" in lib.dt_last_error()
    assert lib.dt_pwconv_affine(p, None, p, p, p, p, None, None, None, 1, 4, 4, 16, 16, 0, 16, 0, None) < 0
    assert b"src1" in lib.dt_last_error()
    assert lib.dt_dwconv3x3_affine(p, p, p, p, p, p, p, p, p, 1, 4, 4, 2048, None) < 0
    assert b"C=2048" in lib.dt_last_error()
    assert lib.dt_dwconv3x3_rows(16, 16) == 1 and lib.dt_dwconv3x3_rows(16, 17) == 2 and lib.dt_dwconv3x3_rows(0, 4) < 0
    assert lib.dt_scse_gates(p, p, p, p, p, p, 1, 1, 16, 32, 4, None) < 0
    assert b"hidden" in lib.dt_last_error()
