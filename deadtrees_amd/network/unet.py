"""MI355X-native U-Net (smp ``Unet`` + ``resnet34`` topology) — the drop-in for ``SemSegment.model``.

Replaces ``smp.Unet(**conf, classes=n)`` built at reference deadtrees/network/segmodel.py:63,85 and
called at :214/:235/:280 and deployment/inference.py:60.  Same module boundary:
``forward(x: f32[B,Cin,H,W]) -> logits f32[B,K,H,W]`` and smp-named ``state_dict``.

Inside, nothing is ATen: every convolution / BatchNorm / ReLU / pool / upsample / concat runs in the
hand-written gfx950 kernels of ``libdeadtrees_hip.so`` through its C ABI (include/deadtrees_hip.h),
NHWC, with all parameters in ONE flat fp32 buffer (HWIO conv weights) so the optimiser and the RCCL
gradient all-reduce work on contiguous ranges.  PyTorch only provides device memory, streams and the
autograd entry point (one ``autograd.Function`` for the whole network; the backward pass is an explicit
hand-scheduled chain, not an autograd graph).

The pieces: ``spec`` (layer list, flat-buffer layout), ``bnview`` (BatchNorm workspace / state layout), ``engine_core``
(launch path, workspaces, weight images, side stream), ``engine_fp32`` / ``engine_bf16`` (the two schedules), ``engine``
(``UNetEngine``), ``module`` (``UNetHIP``, ``EncoderView``, state-dict converters).  This module is the import point.
"""
from .engine import UNetEngine
from .engine_core import BN_EPS, BN_MOMENTUM
from .module import IMAGENET_FILE, EncoderView, UNetHIP, patch_first_conv

__all__ = ["UNetHIP", "UNetEngine", "EncoderView", "patch_first_conv", "IMAGENET_FILE", "BN_EPS", "BN_MOMENTUM"]
