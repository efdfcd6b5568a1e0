"""The bf16 units of the U-Net engine: bf16 activations / weight images, fp32 accumulation, fp32 BatchNorm statistics
and coefficients (the launches of ``engine_core``), fp32 master parameters and gradients; stem and head run in fp32.
``forward_bf16_eval`` / ``forward_bf16_eval_head`` / ``forward_bf16_train`` run them under the forward schedule in
``engine_forward``, ``backward_bf16`` under the reverse schedule in ``engine_backward``.  ``BF16_UNITS`` names them for both."""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace
from typing import Optional

import torch

from .. import _lib
from .bnview import BnView
from .engine_core import _Saved, _pair
from .spec import ConvSpec

_BF = torch.bfloat16


def _conv_kernel_name(desc, cfg, tf=False, bnb=False) -> str:
    """the kernel dt_conv2d_bf16 / dt_conv2d_bf16_bn_bwd launches for `desc`, as the profile names it; cfg = its
    _lib.bf16_config, tf: with an input transform, bnb: with the fused BatchNorm-backward sums"""
    tw, tn, ck, mt = cfg
    t = {False: "false", True: "true"}
    if mt == _lib.BF16_MT_DMA:      # conv_bf16_dma.hip; epilogue: 1 = fused sums, 2 = gradient join, 3 = both
        return f"conv3x3_bf16_dma_kernel<{t[tf]}, {int(bnb) + (2 if desc.accumulate else 0)}>"
    if mt == _lib.BF16_MT_NARROW:   # conv_bf16_narrow.hip
        return f"conv3x3_bf16_narrow_kernel<{desc.C0 // 16}, {desc.Cout // 16}, {t[tf]}, {t[bnb]}>"
    if bnb:
        return "conv_fwd_bf16_kernel (data gradient + BatchNorm-backward sums)"
    return f"conv_fwd_bf16_kernel<{desc.ksize}, {desc.stride}, {tw}, {tn}, {ck}, {mt}, {t[tf]}>"


class Bf16Schedule:
    # ------------------------------------------------------------------ convolution launches
    def _conv_bf16(self, desc, src0, src1, w, out0, out1, stats, in_ss, w_chunked=None):
        cfg = _lib.bf16_config(desc) if w_chunked is not None else None
        if cfg is not None and cfg[3] == _lib.BF16_MT_DMA:      # the LDS-DMA staged kernels read the CHUNKED weight images
            w = w_chunked
        e0 = self._pb()
        self._call("dt_conv2d_bf16", desc, src0, src1, w, out0, out1, stats, *_pair(in_ss))
        if e0 is not None:
            self._pe(e0, _conv_kernel_name(desc, cfg or _lib.bf16_config(desc), tf=bool(in_ss)), *self._conv_work(desc, 2))

    def _stem_bf16(self, x, params, y, stats, B, H, W, Cin):
        """7x7/2 stem of the bf16 path into `y` (bf16) with optional BatchNorm partial statistics -> (stat rows P, the
        statistics buffer | None, the space-to-depth image when there are statistics: the weight gradient reuses it | None).
        Even tiles wider than 32 pixels run on the bf16 MFMA kernels through the 2x2 space-to-depth image
        (dt_stem_s2d_bf16 + a 4x4 window: K = 256 bf16 instead of 147 fp32); anything else on the fp32 stem kernel."""
        lib, stc = self.lib, self.spec.stem
        w7 = stc.w(params)
        h, w_ = y.shape[1], y.shape[2]
        if H % 2 == 0 and W % 2 == 0 and w_ > 16 and stc.cout % 64 == 0 and stc.k == 7 and stc.stride == 2:
            s2d = torch.empty((B, h, w_, 16), dtype=_BF, device=x.device)
            self._call("dt_stem_s2d_bf16", x, s2d, B, H, W, Cin)
            wp = self._buf("stem_w4", 16 * stc.cout * 16, dtype=_BF, device=x.device)
            self._call("dt_stem_pack_weights_bf16", w7, wp, Cin, stc.cout)
            desc = self._desc(B, h, w_, 16, 0, 0, h, w_, stc.cout, 4, 1, 2)
            P = lib.dt_conv2d_bf16_stat_rows(C.byref(desc))
            sbuf = self._buf("bn_stats", lib.dt_bn_stats_floats(P, stc.cout), device=x.device) if stats else None
            self._conv_bf16(desc, s2d, None, wp, y, None, sbuf, None)
            return P, sbuf, s2d if stats else None
        sdesc = self._desc(B, H, W, Cin, 0, 0, h, w_, stc.cout, stc.k, stc.stride, stc.pad)
        P = lib.dt_conv2d_stat_rows(C.byref(sdesc))
        sbuf = self._buf("bn_stats", lib.dt_bn_stats_floats(P, stc.cout), device=x.device) if stats else None
        self._call("dt_conv2d_out_bf16", sdesc, x, w7, y, sbuf)
        return P, sbuf, None

    # ------------------------------------------------------------------ forward units
    def _bn_coeffs_bf16(self, c: ConvSpec, params, bn: BnView, stats, P, count):
        """(scale, shift) of conv c for this pass: from the batch statistics, or (``_batch_stats``: inference, an encoder
        in eval mode — the batch sums of its convolutions are not used) from its running statistics"""
        if self._batch_stats(c):
            return self._bn_finalize(c, params, bn, stats, P, count)
        return self._bn_eval_affine(c, params, bn)

    def _conv_bn_bf16(self, c: ConvSpec, params, bn: BnView, src0, src1, mode0, B, Hin, Win, in_ss=None):
        """y = conv(x) in bf16 -> y, Ho, Wo, (scale, shift).  Every convolution of a training pass (the decoder is on batch
        statistics) writes BatchNorm partial sums — those of a frozen eval-mode encoder too, which ignores them"""
        desc = self._conv_desc(c, src0, src1, mode0, B, Hin, Win)
        stats = P = None
        if self._pass.dec_batch:
            P = self._rows("dt_conv2d_bf16_stat_rows", desc)
            stats = self._buf("bn_stats", self.lib.dt_bn_stats_floats(P, c.cout), device=src0.device)
        y = torch.empty((B, desc.Ho, desc.Wo, c.cout), dtype=_BF, device=src0.device)
        wb, wbc = self._wb
        self._conv_bf16(desc, src0, src1, c.w(wb), y, None, stats, in_ss, w_chunked=c.w(wbc))
        return y, desc.Ho, desc.Wo, self._bn_coeffs_bf16(c, params, bn, stats, P, B * desc.Ho * desc.Wo)

    def _bn_act_bf16(self, y, ss, res=None, res_ss=None, of: Optional[ConvSpec] = None):
        """of: the convolution whose normalise pass this is (recalibration launch record)"""
        Bq, Hq, Wq, Cq = y.shape
        z = torch.empty((Bq, Hq, Wq, Cq), dtype=_BF, device=y.device)
        self._rec_act(of)
        e0 = self._pb() if self._pass.dec_batch else None      # the inference roofline lists the convolutions only
        self._call("dt_bn_act_bf16", y, 0, ss[0], ss[1], res, *_pair(res_ss), z, Bq * Hq * Wq, Cq, 1)
        self._pe(e0, "bn_act_bf16_kernel", 0.0, 2.0 * y.numel() * (2 + (res is not None)))
        return z

    def _resunet_join_bf16(self, blk, params, d, skip, y2, ss2, B, H, W):
        """ResUnet decoder block output under AMP: bf16(relu(y2 * scale2 + shift2) + identity_conv(up(d) | skip) + bias) —
        the 1x1 identity convolution over the virtual (up-sampled, concatenated) input on the bf16 kernels, the join in
        dt_bn_act_bf16 (relu = 2: ReLU on the main branch only)"""
        ic, dev = blk.idc, y2.device
        idy = torch.empty((B, H, W, ic.cout), dtype=_BF, device=dev)
        self._conv_bf16(self._conv_desc(ic, d, skip, 1, B, H, W), d, skip, ic.w(self._wb[0]), idy, None, None, None)
        out = torch.empty((B, H, W, ic.cout), dtype=_BF, device=dev)
        self._call("dt_bn_act_bf16", y2, 0, ss2[0], ss2[1], idy, self._const_vec(1.0, ic.cout, dev), ic.bias(params), out,
                   B * H * W, ic.cout, 2)
        return out

    # ------------------------------------------------------------------ what the shared forward schedule leaves to bf16
    def _stem_fwd_bf16(self, params, bn: BnView, x, B, H, W):
        """stem: bf16 MFMA over the space-to-depth image (fp32-MFMA kernel for odd / tiny tiles), bf16 output, fp32
        statistics -> (activation, Ho, Wo, record for the backward: with the image the weight gradient reuses)"""
        stc = self.spec.stem
        h, w_ = stc.out_size(H), stc.out_size(W)
        y = torch.empty((B, h, w_, stc.cout), dtype=_BF, device=x.device)
        P, stats, s2d = self._stem_bf16(x, params, y, self._pass.dec_batch, B, H, W, x.shape[-1])
        f1 = self._bn_act_bf16(y, self._bn_coeffs_bf16(stc, params, bn, stats, P, B * h * w_), of=stc)
        return f1, h, w_, dict(x=x, y=y, z=f1, Hin=H, Win=W, s2d=s2d)

    def _maxpool_bf16(self, f1, pool, B, h, w_):
        """-> the arg-max map the max-pool backward reads: in every training pass, frozen encoder included"""
        if not self._pass.dec_batch:
            self._call("dt_maxpool3x3s2_bf16", f1, pool, B, h, w_, 64)
            return None
        amax = torch.empty(pool.shape, dtype=torch.uint8, device=f1.device)
        self._call("dt_maxpool3x3s2_bf16_amax", f1, pool, amax, B, h, w_, 64)
        return amax

    def _head_fwd_bf16(self, d, w, bias, logits, am64, am8, B, H, W, cin, K):
        self._call("dt_head_fwd_bf16", d, w, bias, logits, am64, am8, B, H, W, cin, K)

    # ------------------------------------------------------------------ forward
    def _bf16_fwd_weights(self, params):
        self._wb = (self._bf16_weights(params), self._bf16_weights(params, chunked=True))

    def forward_bf16_eval(self, x_nchw: torch.Tensor, params: torch.Tensor, bnstate: torch.Tensor,
                          want_argmax: Optional[str] = None, decoder_only: bool = False):
        """eval-mode forward (``engine_forward``) with bf16 activations/weights and fp32 accumulation (stem and head stay
        fp32) -> (logits, arg-max map | None).
        decoder_only: stop in front of the head and return the bf16 decoder output [B,H,W,16] it would read."""
        self._bf16_fwd_weights(params)
        return self._forward(BF16_UNITS, x_nchw, params, bnstate, False, False, False, want_argmax=want_argmax,
                             decoder_only=decoder_only)

    def forward_bf16_eval_head(self, x_nchw: torch.Tensor, params: torch.Tensor, bnstate: torch.Tensor, labels, lu=None,
                               dist=None, gamma: float = 2.0, counts=None, err=None, want_argmax: bool = False):
        """``forward_bf16_eval`` ending in the fused evaluation head (dt_head_eval_bf16) instead of dt_head_fwd_bf16
        -> what ``ops.head_eval`` returns"""
        return self._forward_eval_head(BF16_UNITS, x_nchw, params, bnstate, labels, lu, dist, gamma, counts, err, want_argmax)

    def forward_bf16_train(self, x_nchw: torch.Tensor, params: torch.Tensor, bnstate: torch.Tensor,
                           enc_training: bool = True, enc_frozen: bool = False, recal: Optional[torch.Tensor] = None):
        """training-mode forward (``engine_forward``, saved for ``backward_bf16``) with bf16 activations / weights, fp32
        accumulation, fp32 BatchNorm statistics (taken from the accumulators), fp32 master parameters -> logits.  Stem and
        head run in fp32.
        enc_frozen: the encoder's weights get no gradient — nothing of it is saved; enc_training=False (only with a
        frozen encoder here: the bf16 path has no frozen-statistics BatchNorm backward) normalises the encoder with its
        running statistics, which stay untouched.
        recal: device float[1] momentum -> BatchNorm recalibration pass, see `forward`: the same kernels on the same
        data as the training forward, nothing kept for backward (`self.saved` stays as it was), Unet: returns None after
        the last BatchNorm's statistics."""
        if recal is not None and (enc_frozen or not enc_training):
            raise RuntimeError("recalibration forward: every BatchNorm layer runs on batch statistics")
        if not enc_training and not enc_frozen:
            raise NotImplementedError("bf16: an encoder in eval mode trains only with frozen weights "
                                      "(model.encoder.requires_grad_(False)); use fp32 for trainable weights on "
                                      "running statistics")
        if self._bf16_images_fused:
            self._bf16_weights_all(params)
        self._bf16_fwd_weights(params)
        return self._forward(BF16_UNITS, x_nchw, params, bnstate, True, enc_training, recal is None, enc_frozen, recal)[0]

    # ------------------------------------------------------------------ backward units
    def _bn_bwd_bf16(self, c: ConvSpec, params, grads, bn: BnView, dout, out_act, y, dres=None, dres_acc=False,
                     virtual_act=False, reduced=None):
        """virtual_act: the activation was never stored, its ReLU mask is recomputed from y * scale + shift.
        reduced = (red, P): the partial sums came out of the kernel that wrote dout"""
        Bq, Hq, Wq, Cq = y.shape
        n_pix = Bq * Hq * Wq
        mean, invstd = bn.mean(c), bn.invstd(c)
        asc, ash = bn.ss(c) if virtual_act else (None, None)
        if reduced is not None:
            red, P = reduced
        else:
            P = self.lib.dt_bn_bwd_rows_bf16(n_pix)
            red = self._buf("bn_red", self.lib.dt_bn_stats_floats(P, Cq), device=y.device)
            e0 = self._pb()
            self._call("dt_bn_bwd_reduce_bf16", dout, out_act, y, mean, invstd, asc, ash, red, n_pix, Cq)
            self._pe(e0, "bn_bwd_reduce_bf16_kernel", 0.0, 2.0 * y.numel() * (2 + (out_act is not None)))
        dy = torch.empty(y.shape, dtype=_BF, device=y.device)
        e0 = self._pb()
        self._call("dt_bn_bwd_apply_bf16", dout, out_act, y, mean, invstd, c.gamma(params), asc, ash, red, P,
                   c.gamma(grads), c.beta(grads), dy, dres, 1 if dres_acc else 0, n_pix, Cq)
        self._pe(e0, "bn_bwd_apply_bf16_kernel", 0.0,
                 2.0 * y.numel() * (3 + (out_act is not None) + (dres is not None) * (2 if dres_acc else 1)))
        return dy

    def _wgrad_bf16(self, c: ConvSpec, grads, src0, src1, mode0, B, Hin, Win, dy, in_ss=None, side=True):
        if side:
            self.launches["wgrad"].append(c.key)
        if side and self.overlap_wgrad_bf16:
            self._on_side(lambda: self._wgrad_bf16(c, grads, src0, src1, mode0, B, Hin, Win, dy, in_ss, side=False),
                          src0, src1, dy)
            return
        C0 = src0.shape[-1]
        C1 = 0 if src1 is None else src1.shape[-1]
        desc = self._desc(B, Hin, Win, C0, C1, mode0, dy.shape[1], dy.shape[2], c.cout, c.k, c.stride, c.pad)
        nbytes = self._rows("dt_conv2d_wgrad_bf16_workspace", desc)
        ws = self._buf("wgrad_ws", nbytes // 4, device=dy.device)
        e0 = self._pb()
        self._call("dt_conv2d_wgrad_bf16", desc, src0, src1, dy, c.w(grads), ws, ws.numel() * 4, *_pair(in_ss))
        if e0 is not None:      # + the fp32 gradient out
            self._pe(e0, "conv_wgrad_bf16_kernel (+ split-K final)", *self._conv_work(desc, 2, 2.0 * c.w_size))

    def _dgrad_bn_bf16(self, c: ConvSpec, dy, B, H, W, out0, bn_conv: ConvSpec, y, bn: BnView, act=None):
        """stride-1 data gradient of conv c into out0 with the BatchNorm-backward reduction of bn_conv (the layer whose raw
        output y has out0's shape) fused; act = stored block output -> the gradient is added to out0 (join) -> (red, P)"""
        Cq = bn_conv.cout
        self.launches["dgrad"].append(c.key)
        desc = self._desc(B, H, W, c.cout, 0, 0, H, W, c.cin, c.k, 1, c.k - 1 - c.pad, 0, 0 if act is None else 1)
        P = self.lib.dt_conv2d_bf16_stat_rows(C.byref(desc))
        red = self._buf("bn_red_fused", self.lib.dt_bn_stats_floats(P, Cq), device=dy.device)
        fuse = bn.fuse(bn_conv, y, act)
        cfg = _lib.bf16_config(desc)
        dma = cfg is not None and cfg[3] == _lib.BF16_MT_DMA
        e0 = self._pb()
        self._call("dt_conv2d_bf16_bn_bwd", desc, dy, c.w(self._wbd[1] if dma else self._wbd[0]), out0, red, fuse)
        if e0 is not None:
            self._pe(e0, _conv_kernel_name(desc, cfg, bnb=True), *self._conv_work(desc, 2, 2.0 * out0.numel()))
        return red, P

    def _dgrad_bf16(self, c: ConvSpec, dy, B, Hin, Win, out0, out1=None, split=0, acc=False):
        self.launches["dgrad"].append(c.key)
        Ho, Wo = dy.shape[1], dy.shape[2]
        pad = c.k - 1 - c.pad
        if c.stride == 1:
            desc = self._desc(B, Ho, Wo, c.cout, 0, 0, Hin, Win, c.cin, c.k, 1, pad, split, 1 if acc else 0)
        else:
            desc = self._desc(B, Hin, Win, c.cout, 0, 2, Hin, Win, c.cin, c.k, 1, pad, split, 1 if acc else 0)
        self._conv_bf16(desc, dy, None, c.w(self._wbd[0]), out0, out1, None, None, w_chunked=c.w(self._wbd[1]))

    # ------------------------------------------------------------------ what the shared reverse schedule leaves to bf16
    def _head_bwd_bf16(self, x, w, dlogits, g, red, B, H, W, cin, K):
        self._call("dt_head_bwd_bf16", x, w, dlogits, g, red, B, H, W, cin, K)

    def _upsample_bwd_bf16(self, dup, g, B, h, w, cx):
        self._call("dt_upsample2x_bwd_bf16", dup, g, B, h, w, cx)

    def _fused_input_grad_bf16(self, blk, below, params, bn: BnView, dy1, d, B, Hh, Ww, frozen):
        """Unet decoder block i >= 1 without a skip (dec4.conv1): data gradient, the 2x2 sums of the up-sampling's backward
        and the BatchNorm-backward sums of the block `below` = (its conv2, its y2) in one launch of the narrow kernel — no
        full-resolution gradient tensor -> (g, (red, P), None), or None where the layer is not covered (the generic chain
        runs)"""
        c1, cx, lib = blk.conv1, blk.in_ch, self.lib
        if d["skip"] is not None:
            return None
        ddesc = self._desc(B, Hh, Ww, c1.cout, 0, 0, Hh, Ww, c1.cin, c1.k, 1, c1.k - 1 - c1.pad, 0, 0)
        if not lib.dt_conv2d_bf16_upsampled_dgrad_supported(C.byref(ddesc)):
            return None
        self.launches["dgrad"].append(c1.key)
        P = lib.dt_conv2d_bf16_stat_rows(C.byref(ddesc))
        red = self._buf("bn_red_up", lib.dt_bn_stats_floats(P, cx), device=dy1.device)
        g = torch.empty_like(d["x"])
        ev = self._pb()
        self._call("dt_conv2d_bf16_upsampled_dgrad", ddesc, dy1, c1.w(self._wbd[0]), g, red, bn.fuse(*below))
        self._pe(ev, f"conv3x3_bf16_narrow_kernel<{c1.cout // 16}, {c1.cin // 16}, false, true, true>",
                 2.0 * 9 * c1.cin * c1.cout * Hh * Ww * B, 2.0 * B * (Hh * Ww * c1.cout + (Hh // 2) * (Ww // 2) * cx * 2))
        return g, (red, P), None

    def _resunet_join_bwd_bf16(self, i, blk, d, g, dy1, B, Hh, Ww, skip_grads):
        """tail of a reversed ResUnet block: dy1 (one-element list, emptied here) and g through conv1 and the identity
        convolution; the two branches' parts are added at full resolution (one rounding), then one up-sample backward"""
        dy1, dev = dy1.pop(), g.device
        ic, cx = blk.idc, blk.in_ch
        sk = 0 if d["skip"] is None else d["skip"].shape[-1]
        n_pix = B * Hh * Ww
        dup = torch.empty((B, Hh, Ww, cx), dtype=_BF, device=dev)
        dup_id = torch.empty((B, Hh, Ww, cx), dtype=_BF, device=dev)
        one = self._const_vec(1.0, max(cx, sk, 8), dev)
        zero = self._const_vec(0.0, max(cx, sk, 8), dev)
        if sk:
            dskip = torch.empty(d["skip"].shape, dtype=_BF, device=dev)
            dskip_id = torch.empty(d["skip"].shape, dtype=_BF, device=dev)
            self._dgrad_bf16(blk.conv1, dy1, B, Hh, Ww, dup, dskip, split=cx)
            self._dgrad_bf16(ic, g, B, Hh, Ww, dup_id, dskip_id, split=cx)
            # gradient of the skip feature = the two branches' parts, one rounding
            self._call("dt_bn_act_bf16", dskip, 0, one, zero, dskip_id, None, None, dskip, n_pix, sk, 0)
            skip_grads[3 - i] = dskip
            self._tr(f"D{i}.dskip", dskip)
            del dskip_id
        else:
            self._dgrad_bf16(blk.conv1, dy1, B, Hh, Ww, dup)
            self._dgrad_bf16(ic, g, B, Hh, Ww, dup_id)
        del dy1
        self._call("dt_bn_act_bf16", dup, 0, one, zero, dup_id, None, None, dup, n_pix, cx, 0)
        del dup_id
        self._tr(f"D{i}.dup", dup)
        gx = torch.empty(d["x"].shape, dtype=_BF, device=dev)
        self._call("dt_upsample2x_bwd_bf16", dup, gx, B, Hh // 2, Ww // 2, cx)
        del dup
        self._tr(f"D{i}.g", gx)
        return gx

    # ------------------------------------------------------------------ backward
    def backward_bf16(self, dlogits: torch.Tensor, params: torch.Tensor, grads: torch.Tensor,
                      saved: Optional[_Saved] = None):
        """reverse pass of forward_bf16_train (``engine_backward``): bf16 activation gradients, fp32 parameter gradients"""
        self._saved_of(saved)      # no saved forward: refused before anything is launched
        self._wbd = (self._bf16_weights(params, dgrad=True), self._bf16_weights(params, dgrad=True, chunked=True))
        self._backward(BF16_UNITS, dlogits, params, grads, saved)

    def _stem_wgrad_bf16(self, stem, dy, grads, B):
        stc, lib, dev = self.spec.stem, self.lib, dy.device
        self.launches["wgrad"].append(stc.key)
        if stem.get("s2d") is not None:
            # space-to-depth form on the bf16 MFMA kernels: dW over 16 taps x 16 channels, gathered back to 7x7
            cin = stem["x"].shape[-1]
            d4 = self._desc(B, dy.shape[1], dy.shape[2], 16, 0, 0, dy.shape[1], dy.shape[2], stc.cout, 4, 1, 2)
            nbytes = self._rows("dt_conv2d_wgrad_bf16_workspace", d4)
            ws = self._buf("wgrad_ws", nbytes // 4, device=dev)
            dw4 = self._buf("stem_dw4", 16 * 16 * stc.cout, device=dev)
            self._call("dt_conv2d_wgrad_bf16", d4, stem["s2d"], None, dy, dw4, ws, ws.numel() * 4, None, None)
            self._call("dt_stem_unpack_wgrad", dw4, stc.w(grads), cin, stc.cout)
        else:
            sdesc = self._desc(B, stem["Hin"], stem["Win"], stem["x"].shape[-1], 0, 0, dy.shape[1], dy.shape[2], stc.cout,
                               stc.k, stc.stride, stc.pad)
            nbytes = lib.dt_conv2d_wgrad_workspace(C.byref(sdesc))
            ws = self._buf("wgrad_ws", nbytes // 4, device=dev)
            self._call("dt_conv2d_wgrad_stem_dy_bf16", sdesc, stem["x"], dy, stc.w(grads), ws, ws.numel() * 4)


def _not_fused(eng, *args):
    """the bf16 path has none of the fused inference forms: the generic block runs"""
    return None


# the bf16 units of the two shared schedules: plain functions of the engine (no engine holds, or is held by, this object)
BF16_UNITS = SimpleNamespace(
    dtype=_BF,
    # ---- forward: unit launchers, the hooks for what is not the same sequence in fp32, the rules read per pass / per block
    conv_bn=Bf16Schedule._conv_bn_bf16, bn_act=Bf16Schedule._bn_act_bf16, stem=Bf16Schedule._stem_fwd_bf16,
    maxpool=Bf16Schedule._maxpool_bf16, fused_encoder_block=_not_fused, fused_unet_block=_not_fused,
    resunet_out=Bf16Schedule._resunet_join_bf16, head=Bf16Schedule._head_fwd_bf16,
    fuse_eval=lambda eng, p: (False, False),
    runs=lambda kind, inference: kind != "efficientunetplusplus",
    # stored activations: none in inference but the last block's output; in a training pass conv1's of an encoder block
    # (DT_BF16_MAT_Z1), and conv1's AND the output of the 64+-channel decoder blocks (DT_BF16_MAT_DEC) so that conv2 / the
    # next conv1 and their weight gradients run the pure LDS-DMA kernels (a DMA cannot transform)
    enc_z1_stored=lambda eng: eng._pass.dec_batch and eng._mat_z1_bf16,
    dec_z1_stored=lambda eng, blk: eng._pass.dec_batch and eng._mat_dec_bf16 and blk.conv2.cout % 64 == 0,
    dec_out_stored=lambda eng, i: eng._pass.dec_batch and eng._mat_dec_bf16 and eng.spec.decoder[i].conv2.cout % 64 == 0,
    saved_tail=lambda p: dict(bf16=True, enc_frozen=p.enc_frozen),
    decoder_output=lambda eng, x, params, bnstate: eng.forward_bf16_eval(x, params, bnstate, decoder_only=True),
    # ---- backward
    bn_bwd=Bf16Schedule._bn_bwd_bf16, wgrad=Bf16Schedule._wgrad_bf16, dgrad=Bf16Schedule._dgrad_bf16,
    dgrad_bn=Bf16Schedule._dgrad_bn_bf16, head_bwd=Bf16Schedule._head_bwd_bf16, upsample_bwd=Bf16Schedule._upsample_bwd_bf16,
    stem_wgrad=Bf16Schedule._stem_wgrad_bf16, fused_input_grad=Bf16Schedule._fused_input_grad_bf16,
    resunet_join=Bf16Schedule._resunet_join_bwd_bf16,
    upsample_bwd_acc="dt_upsample2x_bwd_acc_bf16", upsample_bwd_bn="dt_upsample2x_bwd_bn_bf16",
    channel_sums="dt_channel_sums_bf16", channel_slice="dt_channel_slice_bf16", maxpool_bwd="dt_maxpool3x3s2_bwd_bf16",
    maxpool_bwd_bn="dt_maxpool3x3s2_bwd_bn_bf16",
    # BatchNorm-backward sums in the epilogue of: conv2's data gradient / the up-sampling's backward; the encoder's gradient
    # join; the max-pool backward
    fuse_bn=lambda eng: True, fuse_join=lambda eng: True, fuse_pool=lambda eng: eng._fuse_pool_bn)
