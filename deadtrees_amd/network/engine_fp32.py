"""The fp32 units of the U-Net engine.  ``forward`` / ``forward_eval_head``: convolution + BatchNorm statistics, the
normalise pass, the fused inference forms and the EfficientUnet++ decoder under the forward schedule in ``engine_forward``;
``backward``: BatchNorm backward, weight / data gradients and the fused input gradients under the reverse schedule in
``engine_backward``.  ``FP32_UNITS`` names them for both schedules."""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace
from typing import Optional

import torch

from .. import _lib
from .bnview import BnView
from .engine_core import _Saved, _pair
from .spec import ConvSpec


class Fp32Schedule:
    # ------------------------------------------------------------------ convolution launches
    def _conv_kernel_name(self, desc, transformed: bool = False) -> str:
        """name of the kernel instantiation dt_conv2d launches, spelled like rocprofv3 prints it"""
        tw, tn, ck = C.c_int(), C.c_int(), C.c_int()
        _lib.check(self.lib.dt_conv2d_config(C.byref(desc), C.byref(tw), C.byref(tn), C.byref(ck)), "dt_conv2d_config")
        if ck.value >= 2000:     # its sub-pixel form for the up-sampled input: ck = 2000 + 10 CB + NB
            cb, nbk = (ck.value - 2000) // 10, (ck.value - 2000) % 10
            return f"conv3x3_f32_upc_kernel<{cb}, {nbk}, {'true' if transformed else 'false'}>"
        if ck.value >= 1000:     # the lean narrow-layer kernel (conv_narrow.hip): ck = 1000 + 10 CB + NB
            cb, nbk = (ck.value - 1000) // 10, (ck.value - 1000) % 10
            return f"conv3x3_f32_narrow_kernel<{cb}, {nbk}, {'true' if transformed else 'false'}, false>"
        if tn.value == 16:
            return "conv_fwd_n16_kernel"
        zi = "true" if self.lib.dt_conv2d_uses_zi(C.byref(desc)) else "false"
        tf = "true" if transformed else "false"
        return f"conv_fwd_kernel<{desc.ksize}, {desc.stride}, {tw.value}, {tn.value}, {ck.value}, {zi}, {tf}>"

    @staticmethod
    def _wino_kernel_name(transformed: bool, epi: int) -> str:
        return f"conv3x3_wino_kernel<{'true' if transformed else 'false'}, {epi}>"

    def _use_wino(self, desc, u) -> bool:
        return u is not None and bool(self.lib.dt_conv2d_winograd_supported(C.byref(desc)))

    def _stat_rows(self, desc, u=None) -> int:
        """rows of the BatchNorm partial-statistics buffer the convolution launch for `desc` writes"""
        return self._rows("dt_conv2d_winograd_stat_rows" if self._use_wino(desc, u) else "dt_conv2d_stat_rows", desc)

    def _conv(self, desc, src0, src1, w, out0, out1=None, stats=None, in_ss=None, u=None):
        """u: the layer's Winograd weight image (or None): used when the kernel supports the descriptor"""
        wino = self._use_wino(desc, u)
        e0 = self._pb()
        self._call("dt_conv2d_winograd" if wino else "dt_conv2d", desc, src0, src1, u if wino else w, out0, out1, stats,
                   *_pair(in_ss))
        if e0 is not None:
            name = self._wino_kernel_name(in_ss is not None, 2 if desc.accumulate else 0) if wino else \
                self._conv_kernel_name(desc, in_ss is not None)
            self._pe(e0, name, *self._conv_work(desc))

    # ------------------------------------------------------------------ forward units
    def _conv_bn(self, c: ConvSpec, params, bn: BnView, src0, src1, mode0, B, Hin, Win, in_ss=None):
        """y = conv(x); BN statistics -> per-channel scale/shift in the workspace.  Returns y, Ho, Wo, (scale, shift).
        in_ss: (scale, shift) of the layer that produced src0 when src0 is a RAW conv output whose
        BatchNorm-apply + ReLU is fused into this conv's LDS staging (virtual activation).
        A layer on its running statistics (``_batch_stats``) launches without a statistics buffer; where it is saved, a
        backward may follow: mean / invstd from the running statistics too."""
        desc = self._conv_desc(c, src0, src1, mode0, B, Hin, Win)
        Ho, Wo = desc.Ho, desc.Wo
        y = torch.empty((B, Ho, Wo, c.cout), dtype=torch.float32, device=src0.device)
        u = self._u(c)
        if self._batch_stats(c):
            P = self._stat_rows(desc, u)
            stats = self._buf("bn_stats", self.lib.dt_bn_stats_floats(P, c.cout), device=src0.device)
            self._conv(desc, src0, src1, c.w(params), y, None, stats, in_ss, u=u)
            ss = self._bn_finalize(c, params, bn, stats, P, B * Ho * Wo)
        else:
            self._conv(desc, src0, src1, c.w(params), y, None, None, in_ss, u=u)
            ss = self._bn_eval_affine(c, params, bn)
            p = self._pass
            if p.enc_save if c.index in self._enc_index else p.save:
                self._bn_eval_stats(c, bn)
        return y, Ho, Wo, ss

    def _bn_act(self, y, ss, res=None, res_ss=None, of: Optional[ConvSpec] = None, relu=True, out=None):
        """of: the convolution whose normalise pass this is (recalibration launch record).
        relu: True/1 = ReLU after the residual add, 2 = ReLU on the main branch only (ResUnet decoder), 0 = none"""
        B, H, W, Cc = y.shape
        z = torch.empty_like(y) if out is None else out
        self._rec_act(of)
        e0 = self._pb()
        self._call("dt_bn_act", y, ss[0], ss[1], res, *_pair(res_ss), z, B * H * W, Cc, int(relu))
        self._pe(e0, "bn_act_kernel", 0.0, 4.0 * y.numel() * (2 + (res is not None)))
        return z

    def _conv_affine_direct(self, c: ConvSpec, params, bn: BnView, src0, src1, mode0, B, Hin, Win, relu=True):
        """inference: [relu](bn_eval(conv(x))) in one launch of the direct kernel (dt_conv2d_affine) — the layers that are
        neither Winograd nor narrow layers: stem, stride-2 3x3, 1x1 down-sample.  Returns (activation, Ho, Wo)."""
        desc = self._conv_desc(c, src0, src1, mode0, B, Hin, Win)
        scale, shift = self._bn_eval_affine(c, params, bn)
        z = torch.empty((B, desc.Ho, desc.Wo, c.cout), dtype=torch.float32, device=src0.device)
        e0 = self._pb()
        self._call("dt_conv2d_affine", desc, src0, src1, c.w(params), z, scale, shift, 1 if relu else 0)
        if e0 is not None:
            self._pe(e0, self._conv_kernel_name(desc, False), *self._conv_work(desc))
        return z, desc.Ho, desc.Wo

    def _conv_affine_eval(self, c: ConvSpec, params, bn: BnView, src0, src1, mode0, B, Hin, Win, res=None, in_ss=None):
        """inference: relu(bn_eval(conv(x)) [+ res]) in ONE Winograd launch (dt_conv2d_winograd_affine) — no raw output, no
        bn_act pass.  Returns the activation, or None when the layer is not a Winograd layer (caller: conv + bn_act)."""
        if c.k != 3 or c.stride != 1 or c.pad != 1:
            return None
        desc = self._conv_desc(c, src0, src1, mode0, B, Hin, Win)
        u = self._u(c)
        narrow = res is None and not self._use_wino(desc, u) and bool(self.lib.dt_conv2d_narrow_supported(C.byref(desc)))
        if not narrow and (in_ss is not None or not self._use_wino(desc, u)):
            return None
        scale, shift = self._bn_eval_affine(c, params, bn)
        z = torch.empty((B, Hin, Win, c.cout), dtype=torch.float32, device=src0.device)
        e0 = self._pb()
        if narrow:     # the narrow decoder layers (dec3.conv2, dec4): the lean kernel's inference epilogue
            self._call("dt_conv2d_narrow_affine", desc, src0, c.w(params), z, scale, shift, *_pair(in_ss))
            if e0 is not None:
                self._pe(e0, f"conv3x3_f32_narrow_kernel<{desc.C0 // 16}, {c.cout // 16}, {'true' if in_ss else 'false'}, 4>",
                         *self._conv_work(desc))
            return z
        self._call("dt_conv2d_winograd_affine", desc, src0, src1, u, z, scale, shift, res)
        if e0 is not None:
            self._pe(e0, self._wino_kernel_name(False, 5 if res is not None else 4),
                     *self._conv_work(desc, extra_bytes=4.0 * z.numel() if res is not None else 0.0))
        return z

    # ------------------------------------------------------------------ what the shared forward schedule leaves to fp32
    def _stem(self, params, bn: BnView, x, B, H, W):
        """-> (stem activation, Ho, Wo, record for the backward | None: the inference form stores no raw output)"""
        stc = self.spec.stem
        if self._pass.fuse_enc:     # inference: BatchNorm + ReLU in the stem kernel's epilogue
            return (*self._conv_affine_direct(stc, params, bn, x, None, 0, B, H, W), None)
        y, h, w_, ss = self._conv_bn(stc, params, bn, x, None, 0, B, H, W)
        f1 = self._bn_act(y, ss, of=stc)
        return f1, h, w_, dict(x=x, y=y, z=f1, Hin=H, Win=W)

    def _maxpool(self, f1, pool, B, h, w_):
        """-> the arg-max map the max-pool backward reads: only when the encoder is saved"""
        amax = torch.empty(pool.shape, dtype=torch.uint8, device=f1.device) if self._pass.enc_save else None
        self._call("dt_maxpool3x3s2", f1, pool, amax, B, h, w_, 64)
        return amax

    def _fused_encoder_block(self, blk, params, bn: BnView, xin, B, ch, cw):
        """inference form of a residual block -> (output, Ho, Wo), or None where a layer of it is not covered (the
        generic block runs)"""
        if blk.conv1.stride == 1 and blk.down is None:
            z1 = self._conv_affine_eval(blk.conv1, params, bn, xin, None, 0, B, ch, cw)
            out = None if z1 is None else self._conv_affine_eval(blk.conv2, params, bn, z1, None, 0, B, ch, cw, res=xin)
            if out is not None:
                return out, ch, cw
        if blk.down is not None and blk.conv2.cout % 64 == 0:
            # first block of layers 2-4: relu(bn1(conv1)) and bn_d(down(x)) from the direct kernel's epilogue, the
            # join relu(bn2(conv2) + .) in the Winograd kernel's
            z1, h1, w1 = self._conv_affine_direct(blk.conv1, params, bn, xin, None, 0, B, ch, cw)
            rd, _, _ = self._conv_affine_direct(blk.down, params, bn, xin, None, 0, B, ch, cw, relu=False)
            out = self._conv_affine_eval(blk.conv2, params, bn, z1, None, 0, B, h1, w1, res=rd)
            if out is not None:
                return out, h1, w1
        return None

    def _fused_unet_block(self, blk, params, bn: BnView, d, skip, B, Hin, Win):
        """inference form of a Unet decoder block over up(d) | skip -> its activation, or None (the generic block runs)"""
        z1 = self._conv_affine_eval(blk.conv1, params, bn, d, skip, 1, B, Hin, Win)
        if z1 is not None:
            return self._conv_affine_eval(blk.conv2, params, bn, z1, None, 0, B, Hin, Win)
        # conv1 is neither a Winograd nor a narrow layer (dec3.conv1: 128 -> 32 from two sources): its raw output
        # feeds conv2's lean kernel, which applies bn1 + ReLU while staging AND bn2 + ReLU in its epilogue
        y1, _, _, ss1 = self._conv_bn(blk.conv1, params, bn, d, skip, 1, B, Hin, Win)
        z2 = self._conv_affine_eval(blk.conv2, params, bn, y1, None, 0, B, Hin, Win, in_ss=ss1)
        if z2 is None:
            z2 = self._bn_act(self._conv_bn(blk.conv2, params, bn, y1, None, 0, B, Hin, Win, in_ss=ss1)[0],
                              bn.ss(blk.conv2), of=blk.conv2)
        return z2

    def _resunet_out(self, blk, params, d, skip, y2, ss2, B, H, W):
        """ResUnet decoder block output: relu(y2 * scale2 + shift2) + identity_conv(up(d) | skip) + bias — the 1x1 identity
        convolution over the virtual input, the join in dt_bn_act (relu = 2) with the constant-one scale"""
        ic, dev = blk.idc, y2.device
        idy = torch.empty((B, H, W, ic.cout), dtype=torch.float32, device=dev)
        self._conv(self._conv_desc(ic, d, skip, 1, B, H, W), d, skip, ic.w(params), idy)
        out = self._bn_act(y2, ss2, res=idy, res_ss=(self._const_vec(1.0, ic.cout, dev), ic.bias(params)), of=blk.conv2,
                           relu=2)
        del idy
        return out

    def _head_fwd(self, d, w, bias, logits, am64, am8, B, H, W, cin, K):
        e0 = self._pb()
        self._call("dt_head_fwd", d, w, bias, logits, am64, am8, B, H, W, cin, K)
        self._pe(e0, "head_fwd_kernel", 2.0 * 9 * cin * K * B * H * W, 4.0 * B * H * W * (cin + K))

    def _fuse_eval_rule(self, p):
        """(encoder, decoder) run the inference forms with BatchNorm + ReLU (+ residual) in the convolution's epilogue:
        an eval-mode pass that saves nothing — and the encoder alone when it is frozen and in eval mode under a
        training decoder (nothing of it is saved)"""
        kind, opt = self.spec.decoder_kind, self._fuse_eval_opt and self.winograd
        dec = bool(opt and not p.dec_batch and not p.save and kind not in ("resunet", "unetplusplus"))
        return dec or bool(opt and p.enc_frozen and not p.enc_batch and kind == "unet"), dec

    # ------------------------------------------------------------------ forward
    def forward(self, x_nchw: torch.Tensor, params: torch.Tensor, bnstate: torch.Tensor, training: bool,
                save: bool, want_argmax: Optional[str] = None, nhwc: bool = False, enc_training: Optional[bool] = None,
                enc_frozen: bool = False, recal: Optional[torch.Tensor] = None, decoder_only: bool = False):
        """The forward schedule (``engine_forward``) on the fp32 units -> (logits, arg-max map | None).
        nhwc=True: the input already is the kernels' layout [B,H,W,C] (the tiled-inference gather produces it):
        no NCHW -> NHWC pass.  enc_training: BatchNorm mode of the encoder (stem + layers 1-4; default: `training`) —
        False with training=True is fine-tuning on the encoder's running statistics.  enc_frozen: the encoder's weights
        get no gradient: nothing of the encoder is saved for backward, and an encoder in eval mode runs the fused
        inference form.
        recal: device float[1] momentum -> BatchNorm recalibration pass (`update_bn` of stochastic weight averaging): every
        BatchNorm layer, encoder included, normalises with batch statistics and folds them into its running statistics
        with THAT momentum (dt_bn_finalize_dev); nothing is saved.  With the Unet decoder the pass ends once the last
        BatchNorm's statistics are final — no normalise pass of the last convolution, no head — and returns (None, None).
        decoder_only (inference only): stop in front of the head and return the decoder output [B,H,W,16] it would read
        (``forward_eval_head`` hands it to the fused evaluation head)."""
        if decoder_only and (training or save or recal is not None or enc_training):
            raise RuntimeError("decoder_only forward: inference only (eval-mode BatchNorm, nothing saved)")
        if recal is not None:
            if not training or save or enc_frozen:
                raise RuntimeError("recalibration forward: training statistics, nothing saved, no frozen-encoder form")
            enc_training = True
        self._u_all = self._wino_fwd_weights(params)
        return self._forward(FP32_UNITS, x_nchw, params, bnstate, training, training if enc_training is None else enc_training,
                             save, enc_frozen, recal, want_argmax, nhwc, decoder_only)

    def forward_eval_head(self, x_nchw: torch.Tensor, params: torch.Tensor, bnstate: torch.Tensor, labels, lu=None,
                          dist=None, gamma: float = 2.0, counts=None, err=None, want_argmax: bool = False):
        """eval-mode forward (the inference kernels of ``forward(training=False)``) that ends in the fused evaluation head
        instead of dt_head_fwd -> what ``ops.head_eval`` returns"""
        return self._forward_eval_head(FP32_UNITS, x_nchw, params, bnstate, labels, lu, dist, gamma, counts, err, want_argmax)

    # ------------------------------------------------------------------ EfficientUnet++ decoder (inference only)
    def _pwconv(self, c: ConvSpec, params, bn: BnView, src0, src1, up0, B, H, W, act=False, gate=None, res=None, out=None):
        """1x1 convolution c + eval BatchNorm (bias folded in) [+ Hardswish] [+ res] over the virtual input src0 (up-sampled
        when up0) | src1, gated on load by (gc, s) — one dt_pwconv_affine launch"""
        scale, shift = self._bn_eval_affine(c, params, bn)
        C0 = src0.shape[-1]
        C1 = 0 if src1 is None else src1.shape[-1]
        assert C0 + C1 == c.cin, (c.key, C0, C1, c.cin)
        if out is None:
            out = torch.empty((B, H, W, c.cout), dtype=torch.float32, device=src0.device)
        gc, gs = gate if gate is not None else (None, None)
        e0 = self._pb()
        self._call("dt_pwconv_affine", src0, src1, c.w(params), out, scale, shift, gc, gs, res, B, H, W, C0, C1,
                   1 if up0 else 0, c.cout, 1 if act else 0)
        if e0 is not None:
            n = B * H * W
            self._pe(e0, "pwconv_affine_kernel" + ("<gated>" if gate is not None else ""), 2.0 * n * c.cin * c.cout,
                     4.0 * n * (C0 / (4 if up0 else 1) + C1 + c.cout * (2 if res is not None else 1) + (gate is not None))
                     + 4.0 * c.cin * c.cout)
        return out

    def _mbconv(self, mb, params, bn: BnView, src0, src1, up0, B, H, W):
        """one inverted-residual block (reference efficientunetplusplus/decoder.py:55-60) in four or five launches:
        pw1 (+ Hardswish) -> depthwise (+ Hardswish, sSE logits, pooled partial sums) -> cSE gates -> [skip projection] ->
        pw2 with the scSE gate applied while it stages its input and the residual in its epilogue"""
        lib, dev = self.lib, src0.device
        mid = mb.mid
        a = self._pwconv(mb.pw1, params, bn, src0, src1, up0, B, H, W, act=True)
        scale, shift = self._bn_eval_affine(mb.dw, params, bn)
        P = self._rows("dt_dwconv3x3_rows", H, W)
        b = torch.empty_like(a)
        s = torch.empty((B, H, W), dtype=torch.float32, device=dev)
        pool = torch.empty(B * mid * (1 + P), dtype=torch.float32, device=dev)    # gates [B,mid] | partial rows [B,P,mid]
        gc, part = pool[:B * mid], pool[B * mid:]
        e0 = self._pb()
        self._call("dt_dwconv3x3_affine", a, mb.dw.w(params), scale, shift, mb.sse.w(params), mb.sse.bias(params), b, s,
                   part, B, H, W, mid)
        self._pe(e0, "dwconv3x3_affine_kernel", 2.0 * 9 * a.numel() + 2.0 * a.numel(), 4.0 * (2 * a.numel() + s.numel()))
        del a
        e0 = self._pb()
        self._call("dt_scse_gates", part, mb.cse1.w(params), mb.cse1.bias(params), mb.cse2.w(params), mb.cse2.bias(params),
                   gc, B, P, mid, mb.cse1.cout, H * W)
        self._pe(e0, "scse_gates_kernel", 4.0 * B * mid * mb.cse1.cout, 4.0 * (part.numel() + 2 * mid * mb.cse1.cout))
        if mb.skip is not None:      # the projection lands in the output tensor; pw2 then adds onto it in place
            out = self._pwconv(mb.skip, params, bn, src0, src1, up0, B, H, W)
            return self._pwconv(mb.pw2, params, bn, b, None, False, B, H, W, gate=(gc, s), res=out, out=out)
        assert src1 is None and not up0
        return self._pwconv(mb.pw2, params, bn, b, None, False, B, H, W, gate=(gc, s), res=src0)

    def _forward_effunetpp(self, feats, params, bn: BnView, B):
        """the reference's EfficientUnetPlusPlusDecoder (network/extra/efficientunetplusplus/decoder.py:156-184): the nodes
        and wiring of _forward_unetpp, every node two inverted-residual blocks; conv1 reads the up-sampled lower node and
        the concatenated skip as one virtual input (twice: pw1 and the skip projection)"""
        sp = self.spec
        nodes = {f"f{k}": feats[4 - k] for k in range(5)}     # f0 = deepest encoder feature ... f4 = stem output
        for blk in sp.decoder:
            low = nodes[blk.low]
            H, W = 2 * low.shape[1], 2 * low.shape[2]
            skip = None if not blk.cat else self._cat_channels([nodes[n] for n in blk.cat])[0]
            z = self._mbconv(blk.conv1, params, bn, low, skip, True, B, H, W)
            del skip
            nodes[blk.name] = self._mbconv(blk.conv2, params, bn, z, None, False, B, H, W)
        out = nodes[sp.decoder[-1].name]
        return out, out.shape[1], out.shape[2]

    # ------------------------------------------------------------------ backward units
    def _bn_bwd(self, c: ConvSpec, params, grads, bn: BnView, dout, out_act, y, dres=None, dres_acc=False,
                virtual_act=False, reduced=None):
        """virtual_act: the activation was never stored; its ReLU mask is recomputed from y*scale+shift.
        reduced = (red, P): the partial sums were already produced by the data-gradient kernel that wrote `dout`
        (`_dgrad_bn`), so the reduction pass over (dout, y) is skipped."""
        B, H, W, Cc = y.shape
        n_pix = B * H * W
        mean, invstd = bn.mean(c), bn.invstd(c)
        asc, ash = bn.ss(c) if virtual_act else (None, None)
        if reduced is not None:
            red, P = reduced
        else:
            P = self.lib.dt_bn_bwd_rows(n_pix, Cc)
            red = self._buf("bn_red", self.lib.dt_bn_bwd_red_floats(n_pix, Cc), device=y.device)
            e0 = self._pb()
            self._call("dt_bn_bwd_reduce", dout, out_act, y, mean, invstd, asc, ash, red, n_pix, Cc)
            self._pe(e0, "bn_bwd_reduce_kernel", 0.0, 4.0 * y.numel() * (2 + (out_act is not None)))
        dy = torch.empty_like(y)
        e0 = self._pb()
        # eval-mode (frozen) BatchNorm: y*scale+shift with constant statistics -> dy = g*gamma*invstd, no mean terms
        batch_stats = self._bwd_enc_training if c.index in self._enc_index else self._bwd_training
        self._call("dt_bn_bwd_apply" if batch_stats else "dt_bn_bwd_apply_frozen", dout, out_act, y, mean, invstd,
                   c.gamma(params), asc, ash, red, P, c.gamma(grads), c.beta(grads), dy, dres, 1 if dres_acc else 0,
                   n_pix, Cc)
        # dout + y (+ stored activation) read, dy written (+ residual-branch gradient written, or read-modify-written)
        self._pe(e0, "bn_bwd_apply_kernel", 0.0, 4.0 * y.numel() * (3 + (out_act is not None) + (dres is not None) * (2 if dres_acc else 1)))
        return dy

    def _wgrad(self, c: ConvSpec, grads, src0, src1, mode0, B, Hin, Win, dy, in_ss=None, side=True):
        if side:
            self.launches["wgrad"].append(c.key)
        if side and self.overlap_wgrad:
            self._on_side(lambda: self._wgrad(c, grads, src0, src1, mode0, B, Hin, Win, dy, in_ss, side=False),
                          src0, src1, dy)
            return
        C0 = src0.shape[-1]
        C1 = 0 if src1 is None else src1.shape[-1]
        desc = self._desc(B, Hin, Win, C0, C1, mode0, dy.shape[1], dy.shape[2], c.cout, c.k, c.stride, c.pad)
        e0 = self._pb()
        if self.winograd and self.lib.dt_conv2d_wgrad_winograd_supported(C.byref(desc)):
            # 3x3 stride-1 layers with 64-channel blocks: the Winograd form (conv_wino_wgrad.hip, 1.6-1.75x the direct one)
            nbytes = self.lib.dt_conv2d_wgrad_winograd_workspace(C.byref(desc))
            ws = self._buf("wgrad_ws", nbytes // 4, device=dy.device)
            self._call("dt_conv2d_wgrad_winograd", desc, src0, src1, dy, c.w(grads), ws, ws.numel() * 4, *_pair(in_ss))
            if e0 is not None:
                self._pe(e0, "conv3x3_wino_wgrad_kernel (+ split-K reduce / final)", *self._conv_work(desc))
            return
        nbytes = self._rows("dt_conv2d_wgrad_workspace", desc)
        ws = self._buf("wgrad_ws", nbytes // 4, device=dy.device)
        self._call("dt_conv2d_wgrad", desc, src0, src1, dy, c.w(grads), ws, ws.numel() * 4, *_pair(in_ss))
        if e0 is not None:
            self._pe(e0, "conv_wgrad_stem_kernel (+ reduce)" if c is self.spec.stem else
                     ("conv_wgrad_n16_kernel (+ reduce)" if max(desc.C0 + desc.C1, desc.Cout) <= 32 and min(desc.C0 + desc.C1, desc.Cout) <= 16
                      else "conv_wgrad_kernel (+ split-K reduce)"), *self._conv_work(desc))

    def _dgrad_bn(self, c: ConvSpec, dy, B, H, W, out0, bn_conv: ConvSpec, y, bn: BnView, act=None):
        """stride-1 data gradient of conv `c` into out0 with the BatchNorm-backward reduction of `bn_conv` (the layer
        whose raw output `y` has out0's shape) fused into the epilogue -> (red, P) for _bn_bwd.  act None: plain store,
        virtual activation (mask from y); act = stored block output: the gradient is ADDED to out0 (join) and the
        sums are taken over the joined tensor."""
        Cc = bn_conv.cout
        assert c.stride == 1 and c.cin == Cc and tuple(y.shape) == tuple(out0.shape)
        self.launches["dgrad"].append(c.key)
        desc = self._desc(B, H, W, c.cout, 0, 0, H, W, c.cin, c.k, 1, c.k - 1 - c.pad, 0, 0 if act is None else 1)
        ud = self._u(c, dgrad=True)
        wino = self._use_wino(desc, ud)
        P = self._stat_rows(desc, ud)
        red = self._buf("bn_red_fused", self.lib.dt_bn_stats_floats(P, Cc), device=dy.device)
        fuse = bn.fuse(bn_conv, y, act)
        e0 = self._pb()
        self._call("dt_conv2d_winograd_bn_bwd" if wino else "dt_conv2d_bn_bwd", desc, dy, ud if wino else c.w(self._wd_all),
                   out0, red, fuse)
        if e0 is not None:
            # on top of a plain convolution's traffic: y read (+ the stored output read and the join's second pass)
            name = self._wino_kernel_name(False, 1 if act is None else 3) if wino else self._conv_kernel_name(desc, False)
            self._pe(e0, name, *self._conv_work(desc, extra_bytes=(4.0 if act is None else 8.0) * out0.numel()))
        return red, P

    def _upsampled_dgrad(self, blk, prev_conv: ConvSpec, params, bn: BnView, dy1, y2p, d, B, Hh, Ww):
        """decoder block without a skip: gradient of the block input (low resolution) straight from dy1 — the data
        gradient of conv1 and the backward of the nearest x2 upsample in one sub-pixel kernel, the BatchNorm-backward
        sums of the previous block's conv2 in its epilogue.  -> (g, (red, P), None), or None where the layer shape is
        not covered"""
        c = blk.conv1
        cx = blk.in_ch
        desc = self._desc(B, Hh, Ww, cx, 0, 1, Hh, Ww, c.cout, c.k, c.stride, c.pad, 0, 0)
        if not self.lib.dt_conv2d_upsampled_dgrad_supported(C.byref(desc)):
            return None
        self.launches["dgrad"].append(c.key)
        P = self.lib.dt_conv2d_upsampled_dgrad_rows(C.byref(desc))
        red = self._buf("bn_red_up", self.lib.dt_bn_stats_floats(P, cx), device=dy1.device)
        fuse = bn.fuse(prev_conv, y2p)
        g = torch.empty_like(d["x"])
        ev = self._pb()
        self._call("dt_conv2d_upsampled_dgrad", desc, dy1, c.w(params), g, red, fuse)
        self._pe(ev, "conv3x3_f32_upc_dgrad_kernel", 2.0 * 9 * cx * c.cout * Hh * Ww * B,
                 4.0 * B * Hh * Ww * c.cout + 4.0 * B * (Hh // 2) * (Ww // 2) * cx * 2)
        return g, (red, P), None

    def _wino_upsampled_dgrad(self, blk, prev_conv: ConvSpec, bn: BnView, dy1, y2p, d, B, Hh, Ww, x_only: bool):
        """decoder blocks 1-3: the Winograd data gradient of conv1 with the up-sampling's backward (2x2 sums) and the
        BatchNorm-backward sums of the block below in its epilogue; the skip's gradient from a second launch — or, with a
        frozen encoder (x_only), only the up-sampled channels [0, cx): the skip's gradient is neither computed nor
        written.  -> (g, (red, P), dskip | None), or None where the layer shape is not covered"""
        c1, cx, lib = blk.conv1, blk.in_ch, self.lib
        ddesc = self._desc(B, Hh, Ww, c1.cout, 0, 0, Hh, Ww, c1.cin, c1.k, 1, c1.k - 1 - c1.pad, cx, 0)
        ud = self._u(c1, dgrad=True)
        if ud is None or not lib.dt_conv2d_winograd_upsampled_dgrad_supported(C.byref(ddesc)):
            return None
        self.launches["dgrad"].append(c1.key)
        rows = lib.dt_conv2d_winograd_upsampled_dgrad_x_rows if x_only else lib.dt_conv2d_winograd_upsampled_dgrad_rows
        P = rows(C.byref(ddesc))
        red = self._buf("bn_red_up", lib.dt_bn_stats_floats(P, cx), device=dy1.device)
        fuse = bn.fuse(prev_conv, y2p)
        dskip = None if x_only else torch.empty_like(d["skip"])
        g = torch.empty_like(d["x"])
        ev = self._pb()
        if x_only:
            self._call("dt_conv2d_winograd_upsampled_dgrad_x", ddesc, dy1, ud, g, red, fuse)
            self._pe(ev, self._wino_kernel_name(False, 6) + " (x only)", 2.0 * 9 * cx * c1.cout * Hh * Ww * B,
                     4.0 * B * Hh * Ww * c1.cout + 4.0 * B * (Hh // 2) * (Ww // 2) * cx * 2)
        else:
            self._call("dt_conv2d_winograd_upsampled_dgrad", ddesc, dy1, ud, g, dskip, red, fuse, 3)
            self._pe(ev, self._wino_kernel_name(False, 6), 2.0 * 9 * c1.cin * c1.cout * Hh * Ww * B,
                     4.0 * B * Hh * Ww * (c1.cout + (c1.cin - cx)) + 4.0 * B * (Hh // 2) * (Ww // 2) * cx * 2)
        return g, (red, P), dskip

    def _dgrad(self, c: ConvSpec, dy, B, Hin, Win, out0, out1=None, split=0, acc=False):
        """gradient wrt the conv's logical input [B,Hin,Win,cin] (before virtual upsample handling)."""
        self.launches["dgrad"].append(c.key)
        Ho, Wo = dy.shape[1], dy.shape[2]
        wd = c.w(self._wd_all)     # flipped / transposed image, built at the start of backward
        pad = c.k - 1 - c.pad
        if c.stride == 1:
            desc = self._desc(B, Ho, Wo, c.cout, 0, 0, Hin, Win, c.cin, c.k, 1, pad, split, 1 if acc else 0)
        else:
            assert Hin == 2 * Ho and Win == 2 * Wo
            desc = self._desc(B, Hin, Win, c.cout, 0, 2, Hin, Win, c.cin, c.k, 1, pad, split, 1 if acc else 0)
        self._conv(desc, dy, None, wd, out0, out1, None, u=self._u(c, dgrad=True) if c.stride == 1 else None)

    # ------------------------------------------------------------------ what the shared reverse schedule leaves to fp32
    def _head_bwd(self, x, w, dlogits, g, red, B, H, W, cin, K):
        e0 = self._pb()
        self._call("dt_head_bwd", x, w, dlogits, g, red, B, H, W, cin, K)
        self._pe(e0, "head_bwd_kernel", 4.0 * 9 * cin * K * B * H * W, 4.0 * B * H * W * (2 * cin + K))

    def _upsample_bwd(self, dup, g, B, h, w, cx):
        self._call("dt_upsample2x_bwd", dup, g, 0, B, h, w, cx)

    def _fused_input_grad(self, blk, below, params, bn: BnView, dy1, d, B, Hh, Ww, frozen):
        """Unet decoder block i >= 1: the gradient of the block input from ONE kernel that carries the up-sampling's
        backward and the BatchNorm-backward sums of the block `below` = (its conv2, its y2) in its epilogue -> (g, (red, P),
        dskip | None), or None where no such form covers the layer (the generic chain runs)"""
        if not self._fuse_bn:
            return None
        if d["skip"] is None:
            return self._upsampled_dgrad(blk, below[0], params, bn, dy1, below[1], d, B, Hh, Ww)
        if not self.winograd:
            return None
        # frozen encoder: the form that leaves the skip's gradient out, else (or where it does not apply) the full one
        got = self._wino_upsampled_dgrad(blk, below[0], bn, dy1, below[1], d, B, Hh, Ww, x_only=True) if frozen else None
        if got is None:
            got = self._wino_upsampled_dgrad(blk, below[0], bn, dy1, below[1], d, B, Hh, Ww, x_only=False)
        return got

    def _resunet_join(self, i, blk, d, g, dy1, B, Hh, Ww, skip_grads):
        """tail of a reversed ResUnet block: dy1 (one-element list, emptied here) and g through conv1 and the identity
        convolution; the two branches' up-sampled parts meet in two accumulating up-sample backwards"""
        dy1, dev = dy1.pop(), g.device
        ic, cx = blk.idc, blk.in_ch
        sk = 0 if d["skip"] is None else d["skip"].shape[-1]
        dup = torch.empty((B, Hh, Ww, cx), dtype=torch.float32, device=dev)
        dup_id = torch.empty_like(dup)
        if sk:
            dskip, dskip_id = torch.empty_like(d["skip"]), torch.empty_like(d["skip"])
            self._dgrad(blk.conv1, dy1, B, Hh, Ww, dup, dskip, split=cx)
            self._dgrad(ic, g, B, Hh, Ww, dup_id, dskip_id, split=cx)
            # dskip += dskip_id (the split data-gradient kernels accumulate into their first output only)
            one, zero = self._const_vec(1.0, sk, dev), self._const_vec(0.0, sk, dev)
            self._bn_act(dskip, (one, zero), res=dskip_id, relu=0, out=dskip)
            skip_grads[3 - i] = dskip
            self._tr(f"D{i}.dskip", dskip)
            del dskip_id
        else:
            self._dgrad(blk.conv1, dy1, B, Hh, Ww, dup)
            self._dgrad(ic, g, B, Hh, Ww, dup_id)
        del dy1
        gx = torch.empty_like(d["x"])
        self._call("dt_upsample2x_bwd", dup, gx, 0, B, Hh // 2, Ww // 2, cx)
        self._call("dt_upsample2x_bwd", dup_id, gx, 1, B, Hh // 2, Ww // 2, cx)
        self._tr(f"D{i}.g", gx)      # (the two branches' up-sampled parts are never summed at full resolution: no D{i}.dup)
        return gx

    def _stem_wgrad(self, stem, dy, grads, B):
        self._wgrad(self.spec.stem, grads, stem["x"], None, 0, B, stem["Hin"], stem["Win"], dy)

    # ------------------------------------------------------------------ backward
    def backward(self, dlogits: torch.Tensor, params: torch.Tensor, grads: torch.Tensor, saved: Optional[_Saved] = None):
        """Hand-scheduled reverse pass (``engine_backward``).  Writes every parameter gradient into ``grads`` (flat, same
        layout as ``params``) and calls ``grad_hook(name, lo, hi)`` as each bucket of the flat buffer completes.
        ``saved``: the activations of the forward pass this gradient belongs to (default: the engine's last one)."""
        self._saved_of(saved)      # no saved forward: refused before anything is launched
        # data-gradient weight images of every layer ([tap'][co][ci], taps reversed) in one launch
        self._wd_all = self._buf("wd_all", self.spec.n_params, device=dlogits.device)
        self._weight_images(params, self._wd_all, 0)
        self._ud_all = self._wino_images(self._wd_all, "wino_ud", True) if self.winograd else None
        self._backward(FP32_UNITS, dlogits, params, grads, saved)


# the fp32 units of the two shared schedules: plain functions of the engine (no engine holds, or is held by, this object)
FP32_UNITS = SimpleNamespace(
    dtype=torch.float32,
    # ---- forward: unit launchers, the hooks for what is not the same sequence in bf16, the rules read per pass / per block
    conv_bn=Fp32Schedule._conv_bn, bn_act=Fp32Schedule._bn_act, stem=Fp32Schedule._stem, maxpool=Fp32Schedule._maxpool,
    fused_encoder_block=Fp32Schedule._fused_encoder_block, fused_unet_block=Fp32Schedule._fused_unet_block,
    resunet_out=Fp32Schedule._resunet_out, head=Fp32Schedule._head_fwd, effunetpp=Fp32Schedule._forward_effunetpp,
    fuse_eval=Fp32Schedule._fuse_eval_rule,
    # the decoder kinds it runs: the inverted-residual blocks have inference kernels only
    runs=lambda kind, inference: kind != "efficientunetplusplus" or inference,
    # conv1's activation of an encoder / Unet decoder block is stored (eval-mode passes too); block i's output is (the last
    # one always is): where the NEXT block's conv1 runs on the Winograd kernels
    enc_z1_stored=lambda eng: eng._mat_z1,
    dec_z1_stored=lambda eng, blk: eng._mat_z1 and blk.conv2.cout % 64 == 0,
    dec_out_stored=lambda eng, i: eng._mat_z2 and eng.spec.decoder[i + 1].conv1.cout % 64 == 0,
    saved_tail=lambda p: dict(training=p.dec_batch, enc_training=p.enc_batch, enc_frozen=p.enc_frozen),
    decoder_output=lambda eng, x, params, bnstate: eng.forward(x, params, bnstate, False, save=False, decoder_only=True),
    # ---- backward
    bn_bwd=Fp32Schedule._bn_bwd, wgrad=Fp32Schedule._wgrad, dgrad=Fp32Schedule._dgrad, dgrad_bn=Fp32Schedule._dgrad_bn,
    head_bwd=Fp32Schedule._head_bwd, upsample_bwd=Fp32Schedule._upsample_bwd, stem_wgrad=Fp32Schedule._stem_wgrad,
    fused_input_grad=Fp32Schedule._fused_input_grad, resunet_join=Fp32Schedule._resunet_join,
    upsample_bwd_acc="dt_upsample2x_bwd", upsample_bwd_bn="dt_upsample2x_bwd_bn", channel_sums="dt_channel_sums",
    channel_slice="dt_channel_slice", maxpool_bwd="dt_maxpool3x3s2_bwd", maxpool_bwd_bn="dt_maxpool3x3s2_bwd_bn",
    # BatchNorm-backward sums in the epilogue of: conv2's data gradient / the up-sampling's backward; the encoder's gradient
    # join; the max-pool backward
    fuse_bn=lambda eng: eng._fuse_bn, fuse_join=lambda eng: eng.fuse_join_fp32,
    fuse_pool=lambda eng: eng._fuse_bn and eng._fuse_pool_bn)
