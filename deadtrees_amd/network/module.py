"""``UNetHIP``: the ``nn.Module`` face of the engine — the drop-in for ``SemSegment.model`` — with its autograd entry
point, the ``model.encoder`` view, the smp ``state_dict`` converters, pretrained-encoder loading and the BatchNorm
recalibration (``update_bn``) of stochastic weight averaging."""
from __future__ import annotations

import os
from typing import Optional

import torch
import torch.nn as nn

from .bnview import BnView
from .engine import UNetEngine
from .spec import ConvSpec, build_spec


class _UNetFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, flat, module):
        eng = module.engine
        enc_tr, frozen = module._encoder_training(), module.encoder_frozen
        if module.precision == "bf16" and module.training:
            logits = eng.forward_bf16_train(x, flat.detach(), module.bn_state, enc_training=enc_tr, enc_frozen=frozen)
        else:
            logits, _ = eng.forward(x, flat.detach(), module.bn_state, module.training, save=True, enc_training=enc_tr,
                                    enc_frozen=frozen)
        # the activations belong to THIS autograd node, not to the engine: another grad-enabled forward (a validation
        # step, a second loss term) between this forward and its backward must not replace them
        ctx.saved_acts, eng.saved = eng.saved, None
        ctx.module = module
        module._bn_tracked_inc()
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        m = ctx.module
        grads = m._grad_buffer()
        sv, ctx.saved_acts = ctx.saved_acts, None
        if sv is None:
            raise RuntimeError("UNetHIP: backward through the same forward twice (activations are freed after use)")
        if sv.d.get("bf16"):
            m.engine.backward_bf16(dlogits, m.flat_params.detach(), grads, saved=sv)
        else:
            m.engine.backward(dlogits, m.flat_params.detach(), grads, saved=sv)
        if sv.d.get("enc_frozen"):
            grads[:m.encoder_hi].zero_()     # never written by a frozen backward: no stale gradient reaches .grad
        # a trainer that consumes the flat buffer directly (HipTrainer) opts out of autograd's copy into .grad
        return None, (grads if m.deliver_grad_to_autograd else None), None


IMAGENET_FILE = "resnet34-333f7ec4.pth"     # torchvision's resnet34 weights = smp's resnet34 "imagenet" encoder


def patch_first_conv(w: torch.Tensor, in_channels: int) -> torch.Tensor:
    """smp ``patch_first_conv`` (encoders/_utils.py, smp >= 0.2.1; restated from its published source, unpinned): a
    3-channel pretrained first conv [O,3,k,k] for `in_channels` inputs — C = 1: the sum over the 3 channels; otherwise
    input channel i takes pretrained channel i % 3 and the whole weight is scaled by 3 / C."""
    if in_channels == w.shape[1]:
        return w
    if in_channels == 1:
        return w.sum(1, keepdim=True)
    out = torch.empty((w.shape[0], in_channels) + tuple(w.shape[2:]), dtype=w.dtype)
    for i in range(in_channels):
        out[:, i] = w[:, i % w.shape[1]]
    return out * (w.shape[1] / in_channels)


class EncoderView(nn.Module):
    """``model.encoder``: the resnet34 encoder (stem + layers 1-4) of a ``UNetHIP`` as a parameter-free child module.

    Its tensors live in the owner's flat buffer, so it adds no parameters and no state_dict keys to the model.
    ``train()`` / ``eval()`` set the encoder's BatchNorm mode (the owner's ``train()`` / ``eval()`` recurse into it, as
    torch does); ``requires_grad_(flag)`` freezes / unfreezes the encoder's weights as a whole (the contiguous range
    [0, encoder_hi) of the flat buffer; per-tensor ``requires_grad`` is not supported); ``state_dict()`` /
    ``load_state_dict()`` use smp's encoder key names (``smp_model.encoder``: no ``encoder.`` prefix; torchvision's
    ``fc.*`` is ignored on load)."""

    def __init__(self, owner: "UNetHIP"):
        super().__init__()
        object.__setattr__(self, "_owner_ref", owner)     # not a child module: no recursion, no parameters

    def __setattr__(self, name, value):
        # the reference's MultiStage assigns `m.requires_grad_ = False` to every encoder module: an attribute assignment
        # that changes nothing there — a no-op here too (it must not shadow the method)
        if name == "requires_grad_":
            return
        super().__setattr__(name, value)

    def requires_grad_(self, requires_grad: bool = True):
        self._owner_ref.encoder_frozen = not requires_grad
        return self

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        pass        # the owner's state_dict already holds the encoder's tensors under "encoder.*"

    def _load_from_state_dict(self, *args, **kwargs):
        pass

    def state_dict(self, *args, destination=None, prefix: str = "", keep_vars: bool = False):
        if destination is not None:     # the owner's state_dict recursing: its "encoder.*" keys are already there
            return destination
        sd = self._owner_ref.smp_state_dict()
        out = {}
        for k, v in sd.items():
            if k.startswith("encoder."):
                out[prefix + k[len("encoder."):]] = v
        return out

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """torchvision resnet34 / smp encoder keys (an ``encoder.`` prefix is accepted too); ``fc.*`` ignored.  Every
        encoder tensor must be present with its shape (``num_batches_tracked`` excepted: old torchvision files lack it)."""
        owner = self._owner_ref
        sub = {(k[len("encoder."):] if k.startswith("encoder.") else k): v for k, v in state_dict.items()}
        sub = {k: v for k, v in sub.items() if not k.startswith("fc.")}
        full = owner.smp_state_dict()
        enc_keys = [k[len("encoder."):] for k in full if k.startswith("encoder.")]
        missing = [k for k in enc_keys if k not in sub and not k.endswith("num_batches_tracked")]
        unexpected = [k for k in sub if k not in set(enc_keys)]
        if missing:
            raise RuntimeError(f"encoder state_dict: missing keys {missing[:8]}{'...' if len(missing) > 8 else ''}")
        if strict and unexpected:
            raise RuntimeError(f"encoder state_dict: unexpected keys {unexpected[:8]}")
        for k in enc_keys:
            if k in sub:
                t = torch.as_tensor(sub[k])
                if tuple(t.shape) != tuple(full["encoder." + k].shape):
                    raise RuntimeError(f"size mismatch for encoder.{k}: {tuple(t.shape)} vs "
                                       f"{tuple(full['encoder.' + k].shape)}")
                full["encoder." + k] = t
        owner.load_smp_state_dict(full)
        return nn.modules.module._IncompatibleKeys([], unexpected)


class UNetHIP(nn.Module):
    """Drop-in for ``smp.Unet("resnet34", encoder_depth=5, decoder_channels=(256,128,64,32,16),
    encoder_weights=None, in_channels=C, classes=K)`` on MI355X."""

    def __init__(self, encoder_name: str = "resnet34", encoder_depth: int = 5, encoder_weights=None,
                 decoder_channels=(256, 128, 64, 32, 16), in_channels: int = 3, classes: int = 2,
                 decoder: str = "unet", decoder_use_batchnorm=True, decoder_attention_type=None, squeeze_ratio: int = 1,
                 expansion_ratio: int = 1, **unused):
        """decoder "unet": smp.Unet; "resunet": the reference's in-tree ResUnet (network/extra/resunet/model.py:57-103 —
        residual decoder blocks with a 1x1 identity_conv, 1x1 segmentation head); "unetplusplus": smp.UnetPlusPlus (dense
        nested decoder x_{depth}_{layer}, 3x3 head); "efficientunetplusplus": the reference's in-tree EfficientUnet++ decoder
        on this encoder (network/extra/efficientunetplusplus/decoder.py: the same dense nodes, two inverted-residual blocks
        with scSE each; ``squeeze_ratio`` / ``expansion_ratio`` as there) — INFERENCE ONLY: fp32, eval-mode BatchNorm; a
        training-mode forward, bf16, ``update_bn`` and ``HipTrainer`` raise NotImplementedError (``inference_only``).
        The alternatives run on the fp32 path."""
        super().__init__()
        if decoder_use_batchnorm is not True or decoder_attention_type is not None:
            raise NotImplementedError("only decoder_use_batchnorm=True / decoder_attention_type=None have HIP kernels")
        if encoder_name != "resnet34":
            raise NotImplementedError(f"encoder {encoder_name!r}: only resnet34 has HIP kernels")
        if encoder_depth != 5 or tuple(decoder_channels) != (256, 128, 64, 32, 16):
            raise NotImplementedError("only encoder_depth=5 / decoder_channels=(256,128,64,32,16)")
        self.spec = build_spec(in_channels, classes, decoder, squeeze_ratio, expansion_ratio)
        # no backward and no bf16 kernels for the inverted-residual blocks: such a model only predicts
        self.inference_only = decoder == "efficientunetplusplus"
        self.flat_params = nn.Parameter(torch.zeros(self.spec.n_params, dtype=torch.float32))
        self.register_buffer("bn_state", torch.zeros(BnView.state_floats(self.spec), dtype=torch.float32),
                             persistent=False)
        self.register_buffer("num_batches_tracked", torch.zeros(len(self.spec.convs), dtype=torch.int64),
                             persistent=False)
        self._engine: Optional[UNetEngine] = None
        self._grads: Optional[torch.Tensor] = None
        self.deliver_grad_to_autograd = True
        # "fp32" (BASELINE configs[1]) or "bf16": bf16 activations/weights, fp32 accumulation, fp32 master
        # parameters and optimiser (configs[2]; the AMP setting of the reference's protocol.md:27)
        self.precision = "fp32"
        # model.encoder: the encoder's BatchNorm mode (train / eval) and weight freeze (requires_grad_); adds no parameters
        self.encoder = EncoderView(self)
        self.encoder_frozen = False
        self.encoder_hi = self.spec.buckets[0][1]          # encoder = flat buffer range [0, encoder_hi)
        self._n_enc_convs = sum(c.key.startswith("encoder.") for c in self.spec.convs)
        self.encoder_weights = encoder_weights
        self.reset_parameters()
        if encoder_weights is not None:
            self.init_decoder_smp()
            self.load_encoder_weights(encoder_weights)

    # ------------------------------------------------------------------ pretrained encoder
    @staticmethod
    def imagenet_path() -> str:
        """where ``encoder_weights="imagenet"`` is read from: torch's hub cache (never downloaded here)"""
        return os.path.join(torch.hub.get_dir(), "checkpoints", IMAGENET_FILE)

    @torch.no_grad()
    def load_encoder_weights(self, weights):
        """"imagenet" -> the torchvision resnet34 file in the hub cache; any other string -> a path to a torchvision- or
        smp-encoder-style state_dict; a dict -> that state_dict.  The first conv is patched as smp does for
        in_channels != 3 (``patch_first_conv``)."""
        if isinstance(weights, str):
            path = self.imagenet_path() if weights == "imagenet" else weights
            if not os.path.isfile(path):
                raise FileNotFoundError(f"encoder weights {weights!r}: no file at {path} (nothing is downloaded; place "
                                        f"torchvision's {IMAGENET_FILE} there or pass a state_dict path)")
            sd = torch.load(path, map_location="cpu", weights_only=True)
        else:
            sd = weights
        sd = {(k[len("encoder."):] if k.startswith("encoder.") else k): v for k, v in sd.items()}
        if "conv1.weight" in sd:
            sd["conv1.weight"] = patch_first_conv(torch.as_tensor(sd["conv1.weight"]).float(), self.spec.in_channels)
        self.encoder.load_state_dict(sd, strict=False)

    @torch.no_grad()
    def init_decoder_smp(self):
        """smp's initialisation of decoder and head (what the reference keeps when ``encoder_weights`` is set,
        segmodel.py:87-89): decoder convs kaiming_uniform_(fan_in, relu) with zero bias, BatchNorm 1 / 0, head
        xavier_uniform_ with zero bias.  Draws from torch's global generator."""
        sd = self.smp_state_dict()
        for c in self.spec.convs:
            if c.key.startswith("encoder."):
                continue
            k = c.state_k
            shape = (c.cout, c.w_cin, k, k)
            w = torch.empty(shape)
            if c is self.spec.head:
                nn.init.xavier_uniform_(w)
            else:
                nn.init.kaiming_uniform_(w, mode="fan_in", nonlinearity="relu")
            sd[c.key] = w
            if c.has_bias:
                sd[c.bias_key] = torch.zeros(c.cout)
            if c.bn_key is not None:
                sd[f"{c.bn_key}.weight"] = torch.ones(c.cout)
                sd[f"{c.bn_key}.bias"] = torch.zeros(c.cout)
        self.load_smp_state_dict(sd)

    def _encoder_training(self) -> bool:
        """BatchNorm mode of the encoder for the next forward"""
        return bool(self.training and self.encoder.training)

    def trainable_ranges(self):
        """[(lo, hi)] of the flat buffer that receive gradients and updates; None = all of it"""
        if not self.encoder_frozen:
            return None
        return [(self.encoder_hi, self.spec.n_params)]

    # ------------------------------------------------------------------ init / state_dict
    def reset_parameters(self, seed: Optional[int] = None):
        """Kaiming-normal conv weights (fan_in, gain sqrt 2), zero biases, BN gamma 1 / beta 0 — what the
        reference ends with when ``encoder_weights is None`` (segmodel.py:87-89,432-438)."""
        g = torch.Generator().manual_seed(seed) if seed is not None else None
        sd = {}
        for c in self.spec.convs:
            k = c.state_k
            fan_in = c.w_cin * k * k
            sd[c.key] = torch.randn((c.cout, c.w_cin, k, k), generator=g) * (2.0 / fan_in) ** 0.5
            if c.has_bias:
                sd[c.bias_key] = torch.zeros(c.cout)
            if c.bn_key is not None:
                sd[f"{c.bn_key}.weight"] = torch.ones(c.cout)
                sd[f"{c.bn_key}.bias"] = torch.zeros(c.cout)
                sd[f"{c.bn_key}.running_mean"] = torch.zeros(c.cout)
                sd[f"{c.bn_key}.running_var"] = torch.ones(c.cout)
                sd[f"{c.bn_key}.num_batches_tracked"] = torch.tensor(0)
        self.load_smp_state_dict(sd)

    @torch.no_grad()
    def load_smp_state_dict(self, sd, strict: bool = True):
        """smp/torch layout (OIHW conv weights) -> flat HWIO buffer."""
        flat = torch.zeros(self.spec.n_params, dtype=torch.float32)
        bn = BnView(self.spec, state=torch.zeros(BnView.state_floats(self.spec), dtype=torch.float32))
        nbt = torch.zeros(len(self.spec.convs), dtype=torch.int64)
        missing = []

        def get(k, shape):
            if k not in sd:
                missing.append(k)
                return None
            t = sd[k].detach().to("cpu", torch.float32)
            if tuple(t.shape) != tuple(shape):
                raise RuntimeError(f"size mismatch for {k}: {tuple(t.shape)} vs {tuple(shape)}")
            return t

        for c in self.spec.convs:
            w = get(c.key, (c.cout, c.w_cin, c.state_k, c.state_k))
            if w is not None:
                if c.state_k != c.k:     # 1x1 head held as the centre tap of the 3x3 head kernel
                    full = torch.zeros((c.cout, c.w_cin, c.k, c.k), dtype=torch.float32)
                    full[:, :, c.k // 2, c.k // 2] = w[:, :, 0, 0]
                    w = full
                if c.layout == "hwio":
                    c.w(flat).copy_(w.permute(2, 3, 1, 0).reshape(-1))
                else:
                    c.w(flat).copy_(w.permute(0, 2, 3, 1).reshape(-1))   # head: OHWI
            if c.bn_key is not None:
                for name, dst in (("weight", c.gamma(flat)), ("bias", c.beta(flat)),
                                  ("running_mean", bn.running_mean(c)), ("running_var", bn.running_var(c))):
                    t = get(f"{c.bn_key}.{name}", (c.cout,))
                    if t is not None:
                        dst.copy_(t)
                k = f"{c.bn_key}.num_batches_tracked"
                if k in sd:
                    nbt[c.index] = int(sd[k])
            if c.has_bias:
                t = get(c.bias_key, (c.cout,))
                if t is not None:
                    c.conv_bias(flat).copy_(t)
        if strict and missing:
            raise RuntimeError(f"missing keys in state_dict: {missing[:8]}{'...' if len(missing) > 8 else ''}")
        self.flat_params.data.copy_(flat.to(self.flat_params.device))
        if self._engine is not None:
            self._engine.mark_weights_changed()
        self.bn_state.copy_(bn.state.to(self.bn_state.device))
        self.num_batches_tracked.copy_(nbt.to(self.num_batches_tracked.device))
        return missing

    def smp_state_dict(self, prefix: str = ""):
        """flat HWIO buffer -> smp/torch-named tensors (what ``smp.Unet.state_dict()`` would hold)."""
        flat = self.flat_params.detach().cpu()
        bn = BnView(self.spec, state=self.bn_state.detach().cpu())
        nbt = self.num_batches_tracked.cpu()
        out = {}
        for c in self.spec.convs:
            if c.bn_key is not None:
                out[prefix + c.key] = c.w(flat).reshape(c.k, c.k, c.w_cin, c.cout).permute(3, 2, 0, 1).contiguous()
                if c.has_cbias:
                    out[prefix + c.bias_key] = c.conv_bias(flat).clone()
                out[prefix + f"{c.bn_key}.weight"] = c.gamma(flat).clone()
                out[prefix + f"{c.bn_key}.bias"] = c.beta(flat).clone()
                out[prefix + f"{c.bn_key}.running_mean"] = bn.running_mean(c).clone()
                out[prefix + f"{c.bn_key}.running_var"] = bn.running_var(c).clone()
                out[prefix + f"{c.bn_key}.num_batches_tracked"] = nbt[c.index].clone()
            else:
                out[prefix + c.key] = self._oihw(c.w(flat), c)
                out[prefix + c.bias_key] = c.bias(flat).clone()
        return out

    @staticmethod
    def _oihw(w_flat: torch.Tensor, c: ConvSpec) -> torch.Tensor:
        """flat-buffer weight of a convolution without BatchNorm (head, identity_conv) -> torch OIHW, state_dict size"""
        if c.layout == "hwio":
            w = w_flat.reshape(c.k, c.k, c.cin, c.cout).permute(3, 2, 0, 1)
        else:
            w = w_flat.reshape(c.cout, c.k, c.k, c.cin).permute(0, 3, 1, 2)
        if c.state_k != c.k:
            w = w[:, :, c.k // 2:c.k // 2 + 1, c.k // 2:c.k // 2 + 1]
        return w.contiguous()

    # nn.Module protocol: expose smp keys so Lightning checkpoints stay interchangeable with the reference
    def _save_to_state_dict(self, destination, prefix, keep_vars):
        destination.update(self.smp_state_dict(prefix))

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        sub = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
        try:
            miss = self.load_smp_state_dict(sub, strict=False)
            missing_keys.extend(prefix + m for m in miss)
        except RuntimeError as e:  # size mismatch
            error_msgs.append(str(e))

    def smp_grad_dict(self):
        """parameter gradients under smp names / OIHW layout (parity tests, debugging)."""
        g = self._grad_buffer().detach().cpu()
        out = {}
        for c in self.spec.convs:
            if c.bn_key is not None:
                out[c.key] = c.w(g).reshape(c.k, c.k, c.cin, c.cout).permute(3, 2, 0, 1).contiguous()
                out[f"{c.bn_key}.weight"] = c.gamma(g).clone()
                out[f"{c.bn_key}.bias"] = c.beta(g).clone()
            else:
                out[c.key] = self._oihw(c.w(g), c)
                out[c.key.replace(".weight", ".bias")] = c.bias(g).clone()
        return out

    # ------------------------------------------------------------------ execution
    @property
    def engine(self) -> UNetEngine:
        if self._engine is None:
            self._engine = UNetEngine(self.spec)
        return self._engine

    def _grad_buffer(self) -> torch.Tensor:
        if self._grads is None or self._grads.device != self.flat_params.device:
            self._grads = torch.zeros_like(self.flat_params.data)
        return self._grads

    def _bn_tracked_inc(self):
        if self.training:
            if self.encoder.training:
                self.num_batches_tracked += 1
            else:       # encoder on running statistics: its counters stay
                self.num_batches_tracked[self._n_enc_convs:] += 1

    def _require_gpu(self, x):
        if not x.is_cuda:
            raise RuntimeError("deadtrees_amd.UNetHIP runs only on an MI355X (HIP) device; there is no CPU fallback")
        if self.flat_params.device != x.device:
            raise RuntimeError(f"model on {self.flat_params.device}, input on {x.device}: call model.to(device)")

    def _require_trainable(self, what: str):
        """the inverted-residual blocks have forward inference kernels only: refuse BEFORE anything runs"""
        if self.inference_only:
            raise NotImplementedError(f"{what}: decoder {self.spec.decoder_kind!r} is inference only in this build — its "
                                      "blocks (depthwise 3x3, scSE, Hardswish) have no backward / batch-statistics and no "
                                      "bf16 kernels; use model.eval() with fp32 prediction")

    @property
    def precision(self) -> str:
        return self._precision

    @precision.setter
    def precision(self, value: str):
        if value == "bf16":
            self._require_trainable('precision="bf16" (missing bf16 path)')
        self._precision = value

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.training:
            self._require_trainable("training-mode forward (missing backward path)")
        self._require_gpu(x)
        if self.inference_only:     # never through autograd: there is no backward to hand the graph
            return self.engine.forward(x.float(), self.flat_params.detach(), self.bn_state, False, save=False)[0]
        x = x.float()
        if torch.is_grad_enabled() and self.flat_params.requires_grad:
            return _UNetFunction.apply(x, self.flat_params, self)
        logits, _ = self.engine.forward(x, self.flat_params.detach(), self.bn_state, self.training, save=False,
                                        enc_training=self._encoder_training())
        self._bn_tracked_inc()
        return logits

    @torch.no_grad()
    def predict_classes(self, x: torch.Tensor, dtype: str = "int64", precision: str = "fp32", nhwc: bool = False) -> torch.Tensor:
        """forward + argmax fused in the head kernel (deployment/inference.py:60-62), eval-mode BN.
        precision "bf16": bf16 activations/weights with fp32 accumulation (the AMP setting of the reference's
        training protocol) — class maps agree with fp32 wherever the logit margin exceeds bf16 rounding."""
        if precision == "bf16":
            self._require_trainable('precision="bf16" (missing bf16 path)')
        self._require_gpu(x)
        if precision == "bf16":
            if nhwc:
                x = x.permute(0, 3, 1, 2).contiguous()
            _, am = self.engine.forward_bf16_eval(x.float(), self.flat_params.detach(), self.bn_state, want_argmax=dtype)
            return am
        if precision != "fp32":
            raise ValueError(f"precision {precision!r}: use 'fp32' or 'bf16'")
        was = self.training
        self.eval()
        try:
            _, am = self.engine.forward(x.float(), self.flat_params.detach(), self.bn_state, False, save=False,
                                        want_argmax=dtype, nhwc=nhwc)
        finally:
            self.train(was)
        return am

    @torch.no_grad()
    def predict_logits(self, x: torch.Tensor, precision: str = "fp32", nhwc: bool = False) -> torch.Tensor:
        """the fp32 NCHW logits ``predict_classes`` takes its argmax of (same forward, eval-mode BN, same ``precision`` /
        ``nhwc`` meaning): what the overlap-stitch blend reads"""
        if precision == "bf16":
            self._require_trainable('precision="bf16" (missing bf16 path)')
        self._require_gpu(x)
        if precision == "bf16":
            if nhwc:
                x = x.permute(0, 3, 1, 2).contiguous()
            return self.engine.forward_bf16_eval(x.float(), self.flat_params.detach(), self.bn_state)[0]
        if precision != "fp32":
            raise ValueError(f"precision {precision!r}: use 'fp32' or 'bf16'")
        was = self.training
        self.eval()
        try:
            return self.engine.forward(x.float(), self.flat_params.detach(), self.bn_state, False, save=False, nhwc=nhwc)[0]
        finally:
            self.train(was)

    @torch.no_grad()
    def forward_bf16(self, x: torch.Tensor) -> torch.Tensor:
        """eval-mode logits (fp32 tensor) from the bf16 path"""
        self._require_trainable('precision="bf16" (missing bf16 path)')
        self._require_gpu(x)
        logits, _ = self.engine.forward_bf16_eval(x.float(), self.flat_params.detach(), self.bn_state)
        return logits

    # ------------------------------------------------------------------ BatchNorm recalibration (stochastic weight averaging)
    def _bn_reset_pattern(self) -> torch.Tensor:
        """running_mean = 0 / running_var = 1 for every BatchNorm layer, in the layout of ``bn_state``"""
        pat = BnView(self.spec, state=torch.zeros(BnView.state_floats(self.spec), dtype=torch.float32))
        for c in self.spec.convs:
            if c.bn_key is not None:
                pat.running_var(c).fill_(1.0)
        return pat.state

    @staticmethod
    def _batch_image(batch) -> torch.Tensor:
        """the image tensor of a batch: a tensor, an ``(img, ...)`` tuple / list or the datamodule's dict"""
        if isinstance(batch, dict):
            from .segmodel import create_combined_batch
            batch = create_combined_batch(batch)
        if isinstance(batch, (list, tuple)):
            batch = batch[0]
        if not torch.is_tensor(batch):
            raise TypeError(f"update_bn: cannot find the image tensor of a {type(batch).__name__} batch")
        return batch

    def _recal_state(self):
        """device scalars of a recalibration pass: batch count int64[1] and the momentum float[1] = 1 / count"""
        dev = self.flat_params.device
        st = getattr(self, "_recal_dev", None)
        if st is None or st[0].device != dev:
            st = self._recal_dev = (torch.zeros(1, dtype=torch.int64, device=dev),
                                    torch.ones(1, dtype=torch.float32, device=dev))
        return st

    def recalibrate_batch(self, x: torch.Tensor, precision: Optional[str] = None):
        """one batch of ``update_bn``: advance the device batch count (momentum = 1 / count), then the statistics-only
        forward.  Launches the same kernels with the same arguments for every batch of one shape: capturable."""
        self._require_trainable("update_bn (missing batch-statistics forward)")
        self._require_gpu(x)
        n_dev, mom = self._recal_state()
        eng = self.engine
        eng._call("dt_cma_advance", n_dev, mom)
        params = self.flat_params.detach()
        if (precision or self.precision) == "bf16":
            eng.forward_bf16_train(x, params, self.bn_state, recal=mom)
        else:
            eng.forward(x, params, self.bn_state, True, save=False, recal=mom)

    @torch.no_grad()
    def update_bn(self, batches, precision: Optional[str] = None, to_device=None, _run=None) -> int:
        """``torch.optim.swa_utils.update_bn`` for this model: running means to 0, variances to 1,
        ``num_batches_tracked`` to 0, then one statistics-only forward per batch in which EVERY BatchNorm layer (the
        encoder's too, whatever ``model.encoder.training`` says — torch calls ``model.train()``) normalises with batch
        statistics and folds them into its running statistics with the cumulative momentum 1 / (batches so far).  The
        train / eval flags of the module and of the encoder view come back exactly as found, ``num_batches_tracked``
        ends at the batch count, parameters are not written.  Returns the batch count.

        precision: "fp32" / "bf16" (default: ``self.precision``).  Batches: tensors, ``(img, ...)`` tuples or the
        datamodule's dicts.  One deliberate difference from torch: an empty iterable raises ``ValueError`` BEFORE any
        state changes (torch would leave every BatchNorm at mean 0 / variance 1)."""
        self._require_trainable("update_bn (missing batch-statistics forward)")
        precision = precision or self.precision
        if precision not in ("fp32", "bf16"):
            raise ValueError(f"precision {precision!r}: use 'fp32' or 'bf16'")
        if not self.flat_params.is_cuda:
            raise RuntimeError("deadtrees_amd.UNetHIP runs only on an MI355X (HIP) device; there is no CPU fallback")
        it = iter(batches)
        try:
            first = next(it)
        except StopIteration:
            raise ValueError("update_bn: no batches (the running statistics were left as they are)") from None
        was, enc_was = self.training, self.encoder.training
        n_dev, _ = self._recal_state()
        k = 0
        try:
            self.bn_state.copy_(self._bn_reset_pattern())
            self.num_batches_tracked.zero_()
            n_dev.zero_()
            batch = first
            while True:
                x = self._batch_image(batch)
                if to_device is not None:
                    x = x.to(to_device)
                self._require_gpu(x)
                x = x if x.dtype == torch.float32 else x.float()
                (_run or self.recalibrate_batch)(x, precision)
                k += 1
                try:
                    batch = next(it)
                except StopIteration:
                    break
        finally:
            self.num_batches_tracked.fill_(k)
            self.engine._bn_epoch += 1      # running statistics rewritten on the device: cached eval affines are stale
            self.train(was)
            self.encoder.train(enc_was)
        return k
