"""architecture "efficientunet++" (reference deadtrees/network/segmodel.py:68-71: EfficientUnet++ decoder, here on the
resnet34 encoder) on the HIP kernels, inference only, against tests/effunetpp_ref.py — whose decoder is pinned by executing
the reference's efficientunetplusplus/decoder.py (tests/golden/effunetpp_decoder*.part*.npz, tests/test_effunetpp_host.py)."""
import numpy as np
import pytest
import torch

from effunetpp_ref import make_effunetpp_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(2, 64, 64, 3, 2, 1, 1), (1, 96, 160, 4, 3, 2, 1)]     # B, H, W, C, K, squeeze, expansion: H/32, W/32 odd
_CACHE = {}


def _case(shape):
    """(HIP model, input, fp64 oracle logits, fp32 CPU oracle logits) of a shape — computed once, shared, never written"""
    if shape not in _CACHE:
        from deadtrees_amd.network.unet import UNetHIP
        B, H, W, C, K, sq, ex = shape
        ref = make_effunetpp_oracle(C, K, seed=11, squeeze=sq, expansion=ex)
        m = UNetHIP(in_channels=C, classes=K, decoder="efficientunetplusplus", squeeze_ratio=sq, expansion_ratio=ex)
        m.load_state_dict(ref.state_dict())
        x = torch.randn((B, C, H, W), generator=torch.Generator().manual_seed(12))
        with torch.no_grad():
            y32 = ref(x)
            y64 = ref.double()(x.double())
        _CACHE[shape] = (m.to(DEV).eval(), x, y64, y32)
    return _CACHE[shape]


@pytest.mark.parametrize("shape", SHAPES)
def test_eval_parity_against_fp64_oracle(shape):
    m, x, y64, y32 = _case(shape)
    with torch.no_grad():
        got = m(x.to(DEV)).cpu()
    assert got.shape == y64.shape and got.dtype == torch.float32
    scale = float(y64.abs().max())
    err = float((got.double() - y64).abs().max())
    err32 = float((y32.double() - y64).abs().max())
    print(f"effunet++ eval {shape}: max|err| {err:.3e} = {err / scale:.2e} of max|logit| {scale:.3e}; "
          f"fp32 CPU oracle {err32:.3e} = {err32 / scale:.2e}")
    assert err <= 1e-4 * scale
    assert torch.equal(m.predict_logits(x.to(DEV)).cpu(), got)
    nhwc = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    assert torch.equal(m.predict_logits(nhwc, nhwc=True).cpu(), got)
    for dtype in ("int64", "uint8"):
        cls = m.predict_classes(nhwc, dtype=dtype, nhwc=True).cpu().long()
        assert torch.equal(cls, got.argmax(dim=1))
    top2 = y64.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > 4 * err
    assert bool(sure.any())
    assert torch.equal(cls[sure], y64.argmax(dim=1)[sure])


@pytest.mark.parametrize("shape", SHAPES[:1])
def test_an_images_logits_do_not_depend_on_its_batch(shape):
    m, x, _, _ = _case(shape)
    x = torch.randn((3,) + tuple(x.shape[1:]), generator=torch.Generator().manual_seed(15)).to(DEV)
    with torch.no_grad():
        assert torch.equal(m(x)[1:2], m(x[1:2].contiguous()))


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_eval_head_counts_equal_the_confusion_matrix_of_predict_classes(shape):
    from deadtrees_amd import ops
    m, x, _, _ = _case(shape)
    B, H, W, C, K = shape[:5]
    g = torch.Generator().manual_seed(13)
    labels = torch.randint(0, K, (B, H, W), generator=g).to(DEV)
    lu = torch.randint(0, 2, (B, H, W), generator=g).to(DEV)
    _, counts, am, err = m.engine.forward_eval_head(x.to(DEV), m.flat_params.detach(), m.bn_state, labels, lu, want_argmax=True)
    cls = m.predict_classes(x.to(DEV), dtype="uint8")
    want, _ = ops.confusion_matrix(cls, labels, lu, K=K)
    assert int(err) == 0 and torch.equal(am, cls) and torch.equal(counts, want)
    assert int(counts[0].sum()) == B * H * W


def test_training_mode_forward_raises_on_the_device_too():
    m, x, _, _ = _case(SHAPES[0])
    m.train()
    try:
        with pytest.raises(NotImplementedError):
            m(x.to(DEV))
        with pytest.raises(NotImplementedError):
            m.engine.forward(x.to(DEV), m.flat_params.detach(), m.bn_state, True, save=False)
    finally:
        m.eval()


def test_end_to_end_tiled_inference_from_a_checkpoint(tmp_path):
    from deadtrees_amd.deployment.inference import PyTorchInference
    from deadtrees_amd.deployment.stats import RasterStats
    from deadtrees_amd.deployment.tiler import infer_tile
    from deadtrees_amd.trainer import checkpoint_writer
    m = _case(SHAPES[0])[0]
    path = tmp_path / "effunetpp.ckpt"
    checkpoint_writer(m)(str(path))
    inf = PyTorchInference(str(path))
    H, W = 160, 224
    raster = np.random.default_rng(14).integers(0, 256, (4, H, W), dtype=np.uint8)
    kw = dict(subtile=64, device=DEV, overlap=16, blend="average", return_probs=True, stats=True)
    a = infer_tile(inf, raster, batch_size=2, **kw)
    b = infer_tile(inf, raster, batch_size=5, **kw)
    assert len(a) == 3 and isinstance(a[2], RasterStats)
    assert a[0].dtype == np.uint8 and a[0].shape == (H, W)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[0], np.asarray(a[1]).argmax(axis=0))
    assert a[2].total == H * W and np.array_equal(a[2].counts, b[2].counts)
