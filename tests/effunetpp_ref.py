"""Torch-primitive restatement of the reference's EfficientUnet++ decoder on the ResNet-34 encoder (reference
segmodel.py:68-71, architecture "efficientunet++"; decoder: network/extra/efficientunetplusplus/decoder.py).

TEST INFRASTRUCTURE, the role oracle/unetpp_ref.py plays for Unet++.  ``tests/make_golden_effunetpp.py`` EXECUTES the
reference's ``EfficientUnetPlusPlusDecoder`` unmodified (loaded by file path) on a seeded feature pyramid and stores its
state_dict, inputs and eval-mode output in ``tests/golden/effunetpp_decoder*.part*.npz``;
``tests/test_effunetpp_host.py`` checks this restatement against them (same state_dict names and shapes, same output).
So the block — 1x1, BN, Hardswish, depthwise 3x3, BN, Hardswish, scSE, 1x1, BN, plus the input or its 1x1 + BN projection
— and the dense wiring are PINNED by execution of the reference; the encoder and the 3x3 head stay as in unet_ref.py.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.unet_ref import DECODER_CHANNELS, ResNet34Encoder


class SCSERef(nn.Module):
    """x * cSE(x) + x * sSE(x); the indices of the two nn.Sequential match the reference's (pool at 0, sigmoid last)"""

    def __init__(self, ch: int, reduction: int):
        super().__init__()
        self.cSE = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(ch, ch // reduction, 1), nn.ReLU(),
                                 nn.Conv2d(ch // reduction, ch, 1), nn.Sigmoid())
        self.sSE = nn.Sequential(nn.Conv2d(ch, 1, 1), nn.Sigmoid())

    def forward(self, x):
        return x * self.cSE(x) + x * self.sSE(x)


class InvertedResidualRef(nn.Module):
    def __init__(self, cin: int, cout: int, expansion_ratio: int = 1, squeeze_ratio: int = 1):
        super().__init__()
        mid = expansion_ratio * cin
        self.same_shape = cin == cout
        self.block = nn.Sequential(
            nn.Conv2d(cin, mid, 1), nn.BatchNorm2d(mid), nn.Hardswish(),
            nn.Conv2d(mid, mid, 3, padding=1, groups=mid), nn.BatchNorm2d(mid), nn.Hardswish(),
            SCSERef(mid, squeeze_ratio),
            nn.Conv2d(mid, cout, 1), nn.BatchNorm2d(cout))
        if not self.same_shape:
            self.skip_conv = nn.Sequential(nn.Conv2d(cin, cout, 1), nn.BatchNorm2d(cout))

    def forward(self, x):
        r = self.block(x)
        return (x if self.same_shape else self.skip_conv(x)) + r


class EffDecoderBlockRef(nn.Module):
    def __init__(self, in_ch, skip_ch, out_ch, squeeze_ratio=1, expansion_ratio=1):
        super().__init__()
        self.conv1 = InvertedResidualRef(in_ch + skip_ch, out_ch, expansion_ratio, squeeze_ratio)
        self.conv2 = InvertedResidualRef(out_ch, out_ch, expansion_ratio, squeeze_ratio)

    def forward(self, x, skip=None):
        x = F.interpolate(x, scale_factor=2, mode="nearest")
        if skip is not None:
            x = torch.cat([x, skip], dim=1)
        return self.conv2(self.conv1(x))


class EfficientUnetPlusPlusDecoderRef(nn.Module):
    def __init__(self, encoder_channels, decoder_channels=DECODER_CHANNELS, squeeze_ratio=1, expansion_ratio=1):
        super().__init__()
        enc = list(encoder_channels[1:])[::-1]
        self.in_channels = [enc[0]] + list(decoder_channels[:-1])
        self.skip_channels = list(enc[1:]) + [0]
        self.out_channels = list(decoder_channels)
        kw = dict(squeeze_ratio=squeeze_ratio, expansion_ratio=expansion_ratio)
        blocks = {}
        for l in range(len(self.in_channels) - 1):
            for d in range(l + 1):
                if d == 0:
                    ic, sc, oc = self.in_channels[l], self.skip_channels[l] * (l + 1), self.out_channels[l]
                else:
                    ic, sc, oc = self.skip_channels[l - 1], self.skip_channels[l] * (l + 1 - d), self.skip_channels[l]
                blocks[f"x_{d}_{l}"] = EffDecoderBlockRef(ic, sc, oc, **kw)
        blocks[f"x_0_{len(self.in_channels) - 1}"] = EffDecoderBlockRef(self.in_channels[-1], 0, self.out_channels[-1], **kw)
        self.blocks = nn.ModuleDict(blocks)
        self.depth = len(self.in_channels) - 1

    def forward(self, *features):
        features = features[1:][::-1]
        dense = {}
        for li in range(len(self.in_channels) - 1):
            for d in range(self.depth - li):
                if li == 0:
                    dense[f"x_{d}_{d}"] = self.blocks[f"x_{d}_{d}"](features[d], features[d + 1])
                else:
                    l = d + li
                    cat = torch.cat([dense[f"x_{i}_{l}"] for i in range(d + 1, l + 1)] + [features[l + 1]], dim=1)
                    dense[f"x_{d}_{l}"] = self.blocks[f"x_{d}_{l}"](dense[f"x_{d}_{l - 1}"], cat)
        dense[f"x_0_{self.depth}"] = self.blocks[f"x_0_{self.depth}"](dense[f"x_0_{self.depth - 1}"])
        return dense[f"x_0_{self.depth}"]


class EffUNetPPR34Ref(nn.Module):
    """the reference's ``EfficientUnetPlusPlus`` (model.py:55-92) with the resnet34 encoder, from torch primitives"""

    def __init__(self, in_channels: int = 3, classes: int = 2, squeeze_ratio: int = 1, expansion_ratio: int = 1):
        super().__init__()
        self.encoder = ResNet34Encoder(in_channels)
        self.decoder = EfficientUnetPlusPlusDecoderRef(self.encoder.out_channels, DECODER_CHANNELS, squeeze_ratio,
                                                       expansion_ratio)
        self.segmentation_head = nn.Sequential(nn.Conv2d(DECODER_CHANNELS[-1], classes, 3, padding=1, bias=True))

    def forward(self, x):
        return self.segmentation_head(self.decoder(*self.encoder(x)))


def randomize_(m: nn.Module, g: torch.Generator, gain: float = 2.0) -> nn.Module:
    """seeded, non-trivial weights: convolutions N(0, gain / fan_in) (2 = Kaiming) with biases, perturbed BatchNorm
    parameters and running statistics"""
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.Conv2d):
                fan_in = mod.weight[0].numel()
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=g) * (gain / fan_in) ** 0.5)
                if mod.bias is not None:
                    mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.1)
            elif isinstance(mod, nn.BatchNorm2d):
                mod.weight.copy_(1.0 + 0.2 * torch.randn(mod.weight.shape, generator=g))
                mod.bias.copy_(0.1 * torch.randn(mod.bias.shape, generator=g))
                mod.running_mean.copy_(0.1 * torch.randn(mod.running_mean.shape, generator=g))
                mod.running_var.copy_(1.0 + 0.2 * torch.rand(mod.running_var.shape, generator=g))
    return m


def make_effunetpp_oracle(in_channels: int = 3, classes: int = 2, seed: int = 0, squeeze: int = 1,
                          expansion: int = 1) -> EffUNetPPR34Ref:
    """Encoder and head as unet_ref.make_oracle draws them (Kaiming, gain 2); the decoder's convolutions with gain 0.5.
    Why: every inverted-residual block ADDS its branch to its input and neither its last 1x1 nor its skip projection is
    followed by an activation, so with Kaiming's ReLU gain each of the 22 blocks multiplies the variance by about 4: the
    logits reach 1e5, the scSE sigmoids see arguments of 1e4 and act as step functions, and the fp32 CPU run of this very
    module is then 1e-2 * max|logit| away from its fp64 run — no parity bound can be checked on such a function.  With gain
    0.5 the activations stay O(10) like a trained network's and fp32 sits 1.5e-6 from fp64 (measured, 2x3x64x64)."""
    m = EffUNetPPR34Ref(in_channels, classes, squeeze, expansion)
    g = torch.Generator().manual_seed(seed)
    randomize_(m.encoder, g)
    randomize_(m.decoder, g, gain=0.5)
    randomize_(m.segmentation_head, g)
    return m.eval()
