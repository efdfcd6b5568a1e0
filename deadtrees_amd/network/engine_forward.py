"""The forward schedule of the U-Net engine, once for both precisions: the driver, the input check and layout pass, the
BatchNorm workspace and the eval-affine cache, stem and max-pool, the encoder loop over one residual block, the three
trainable decoders (dense Unet++, Unet block, ResUnet block), the head tail, the records for the backward and the fused
evaluation head.

What differs between fp32 and bf16 comes in through ``u``, the units object of the pass (``engine_fp32.FP32_UNITS`` /
``engine_bf16.BF16_UNITS``: the unit launchers of that precision as plain functions of the engine, one parameter list per
role; the rules that say which activations are stored; the hooks for the stretches that are not the same sequence: stem,
max-pool, the fused inference forms, the ResUnet block output, the head).

The BatchNorm mode of the pass is ONE record, ``self._pass`` (``engine_core._Pass``), set here and read by the units: a
layer normalises with batch statistics or with its running statistics by whether it is in ``_enc_index``
(``_batch_stats``) — the rule the backward uses.  Every pass sets its own record, ``_recal`` and ``_affine_fresh`` before it
launches anything: nothing of one pass is seen by the next.

Tensor lifetimes are part of the schedule: a block's raw outputs are locals of the block's function and go with it unless
the pass is saved; ``feats`` holds the encoder features to the end of the decoder."""
from __future__ import annotations

from typing import Optional

import torch

from .bnview import BnView
from .engine_core import _Pass, _Saved


class ForwardSchedule:
    def _forward(self, u, x_in: torch.Tensor, params: torch.Tensor, bnstate: torch.Tensor, dec_batch: bool,
                 enc_batch: bool, save: bool, enc_frozen: bool = False, recal: Optional[torch.Tensor] = None,
                 want_argmax: Optional[str] = None, nhwc: bool = False, decoder_only: bool = False):
        """one forward pass on the units `u` (whose weight images the caller has prepared) -> (logits [B,K,H,W] fp32,
        arg-max map or None); the decoder output in front of the head when `decoder_only`; (None, None) after a
        recalibration pass of the Unet decoder.
        dec_batch / enc_batch: decoder / encoder (stem + layers 1-4) BatchNorm on batch statistics, else on the running
        ones.  save: keep what the backward needs in ``self.saved`` — of the encoder only when its weights are not frozen
        (`enc_frozen`).  recal: device float[1] momentum -> BatchNorm recalibration pass (see ``forward``)."""
        sp = self.spec
        self._recal = None
        if not u.runs(sp.decoder_kind, not (dec_batch or enc_batch or save or enc_frozen or recal is not None)):
            raise NotImplementedError(f"decoder {sp.decoder_kind!r} is inference only: its inverted-residual blocks have no "
                                      "batch-statistics forward, no backward and no bf16 kernels (fp32, eval-mode "
                                      "BatchNorm, nothing saved)")
        if recal is not None and (recal.dtype != torch.float32 or recal.device != x_in.device):
            raise RuntimeError("recalibration forward: the momentum is a float32 tensor on the input's device")
        x_in, B, H, W = self._fwd_check_input(x_in, nhwc)
        dev = x_in.device
        if recal is not None:
            self._recal, self.recal_launches = recal, []
        p = self._pass = _Pass(dec_batch, enc_batch, save, save and not enc_frozen, enc_frozen)
        p.fuse_enc, p.fuse_dec = u.fuse_eval(self, p)
        sv = _Saved() if save else None
        bn = BnView(sp, self._fwd_bn_workspace(sv, params, bnstate, dev), bnstate)

        if nhwc:
            x = x_in
        else:
            x = torch.empty((B, H, W, sp.in_channels), dtype=torch.float32, device=dev)
            self._call("dt_nchw_to_nhwc", x_in, x, B, sp.in_channels, H, W)

        # ---- stem, max-pool
        f1, h, w_, rec = u.stem(self, params, bn, x, B, H, W)
        if p.enc_save:
            sv.d["stem"] = rec
        del rec
        hp, wp = (h + 2 - 3) // 2 + 1, (w_ + 2 - 3) // 2 + 1
        pool = torch.empty((B, hp, wp, 64), dtype=u.dtype, device=dev)
        amax = u.maxpool(self, f1, pool, B, h, w_)
        if p.enc_save:
            sv.d["pool"] = dict(amax=amax, H=h, W=w_)
        del amax
        self._tr("pool", pool)

        # ---- encoder: feats = [f1, f2, f3, f4, f5]
        feats = [f1]
        cur, ch, cw = pool, hp, wp
        del pool
        for li, blocks in enumerate(sp.layers):
            for bi, blk in enumerate(blocks):
                got = u.fused_encoder_block(self, blk, params, bn, cur, B, ch, cw) if p.fuse_enc else None
                if got is not None:
                    cur, ch, cw = got
                    continue
                rec, cur, ch, cw = self._fwd_encoder_block(u, blk, params, bn, cur, B, ch, cw)
                if p.enc_save:
                    sv.d[f"L{li}B{bi}"] = rec
                del rec
            feats.append(cur)

        # ---- decoder
        if sp.decoder_kind == "unetplusplus":
            d = self._fwd_unetpp(u, feats, params, bn, B, sv)
        elif sp.decoder_kind == "efficientunetplusplus":
            d = u.effunetpp(self, feats, params, bn, B)[0]
        else:
            d = self._fwd_unet_decoder(u, feats, ch, cw, params, bn, B, sv)
            if d is None:                       # recalibration: every BatchNorm's statistics are final, nothing else to launch
                self._recal = None
                return None, None
        if decoder_only:
            return d

        # ---- head, records for the backward
        dh, dw = d.shape[1], d.shape[2]
        out = self._fwd_head(u, d, params, B, dh, dw, want_argmax)
        if save:
            sv.d["head"] = dict(x=d, H=dh, W=dw)
            sv.d["B"] = B
            sv.d.update(u.saved_tail(p))
            self.saved = sv
        return out

    # ------------------------------------------------------------------ the pieces, in the order of the pass
    def _fwd_check_input(self, x_in: torch.Tensor, nhwc: bool):
        """-> (contiguous input, B, H, W); nhwc: the input already is the kernels' layout [B,H,W,C]"""
        cin = self.spec.in_channels
        if x_in.dim() != 4 or x_in.shape[3 if nhwc else 1] != cin:
            raise RuntimeError(f"expected input {f'[B,H,W,{cin}]' if nhwc else f'[B,{cin},H,W]'}, got {tuple(x_in.shape)}")
        B, H, W = (x_in.shape[0], x_in.shape[1], x_in.shape[2]) if nhwc else (x_in.shape[0], x_in.shape[2], x_in.shape[3])
        if H % 32 or W % 32:
            raise RuntimeError(f"H and W must be divisible by 32 (encoder depth 5), got {H}x{W}")
        if x_in.dtype != torch.float32 or not x_in.is_cuda:
            raise RuntimeError("input must be a float32 CUDA/HIP tensor")
        return x_in.contiguous(), B, H, W

    def _fwd_bn_workspace(self, sv: Optional[_Saved], params, bnstate, dev) -> torch.Tensor:
        """the BatchNorm workspace of the pass (scale / shift / mean / invstd of every layer) — a private copy when the
        pass is saved: the backward reads mean / invstd — and the eval-affine cache: repeated inference calls (tiled
        prediction) skip the 46 eval-mode scale / shift launches while neither the parameters nor the running statistics
        changed (torch's version counters + the epochs of the raw device writes)"""
        p, n = self._pass, BnView.ws_floats(self.spec)
        if sv is not None:
            bnws = sv.d["bnws"] = torch.empty(n, dtype=torch.float32, device=dev)
        else:
            bnws = self._buf("bnws", n, device=dev)
        batch = p.dec_batch or p.enc_batch
        if batch:
            self._bn_epoch += 1         # running statistics are rewritten on the device
        akey = None if (batch or p.save) else (params.data_ptr(), params._version, self._weights_epoch, bnstate.data_ptr(),
                                               bnstate._version, self._bn_epoch, bnws.data_ptr())
        self._affine_fresh = akey is not None and self._ws.get("affine_key") == akey
        self._ws["affine_key"] = akey
        return bnws

    def _fwd_encoder_block(self, u, blk, params, bn: BnView, xin, B, ch, cw):
        """one residual block -> (record for the backward when the encoder is saved, output, Ho, Wo).  z1 = relu(bn1(y1)) is
        virtual — conv2 applies it while staging y1 — unless the units store it"""
        y1, h1, w1, ss1 = u.conv_bn(self, blk.conv1, params, bn, xin, None, 0, B, ch, cw)
        z1 = u.bn_act(self, y1, ss1, of=blk.conv1) if u.enc_z1_stored(self) else None
        y2, h2, w2, ss2 = u.conv_bn(self, blk.conv2, params, bn, y1 if z1 is None else z1, None, 0, B, h1, w1,
                                    in_ss=ss1 if z1 is None else None)
        if blk.down is not None:
            yd, _, _, ssd = u.conv_bn(self, blk.down, params, bn, xin, None, 0, B, ch, cw)
            out = u.bn_act(self, y2, ss2, res=yd, res_ss=ssd, of=blk.conv2)
        else:
            yd = None
            out = u.bn_act(self, y2, ss2, res=xin, of=blk.conv2)
        rec = dict(x=xin, y1=y1, z1=z1, y2=y2, yd=yd, out=out, Hin=ch, Win=cw, H=h2, W=w2) if self._pass.enc_save else None
        return rec, out, h2, w2

    def _fwd_unetpp(self, u, feats, params, bn: BnView, B, sv: Optional[_Saved]):
        """dense decoder of smp.UnetPlusPlus (wiring: reference network/extra/efficientunetplusplus/decoder.py:156-184):
        every node x_{d}_{l} = DecoderBlock(up x2 of its lower node, cat of the nodes / encoder feature on its level).
        Node outputs are stored activations (they feed several consumers); conv2 reads conv1's raw output with the
        BatchNorm + ReLU applied while staging, like everywhere else."""
        sp = self.spec
        nodes = {f"f{k}": feats[4 - k] for k in range(5)}     # f0 = deepest encoder feature ... f4 = stem output
        for blk in sp.decoder:
            low = nodes[blk.low]
            skip, parts = (None, []) if not blk.cat else self._cat_channels([nodes[n] for n in blk.cat])
            y1, h1, w1, ss1 = u.conv_bn(self, blk.conv1, params, bn, low, skip, 1, B, 2 * low.shape[1], 2 * low.shape[2])
            y2, h2, w2, ss2 = u.conv_bn(self, blk.conv2, params, bn, y1, None, 0, B, h1, w1, in_ss=ss1)
            z2 = u.bn_act(self, y2, ss2, of=blk.conv2)
            if sv is not None:
                sv.d["P" + blk.name] = dict(x=low, skip=skip, parts=parts, y1=y1, y2=y2, z2=z2, H=h1, W=w1)
            nodes[blk.name] = z2
        return nodes[sp.decoder[-1].name]

    def _fwd_unet_decoder(self, u, feats, dh, dw, params, bn: BnView, B, sv: Optional[_Saved]):
        """the five blocks of the Unet / ResUnet decoder over the encoder features -> the last block's activation, or None
        where a recalibration pass ended inside the last Unet block"""
        sp, p = self.spec, self._pass
        d, d_ss = feats[4], None      # d_ss: (scale, shift) when d is a raw convolution output with a virtual activation
        skips = [feats[3], feats[2], feats[1], feats[0], None]
        for i, blk in enumerate(sp.decoder):
            skip, Hin, Win = skips[i], 2 * dh, 2 * dw
            if sp.decoder_kind == "resunet":
                rec, d = self._fwd_resunet_block(u, i, blk, params, bn, d, skip, B, Hin, Win)
            else:
                z2 = u.fused_unet_block(self, blk, params, bn, d, skip, B, Hin, Win) if p.fuse_dec and d_ss is None else None
                if z2 is not None:
                    rec, d = None, z2
                else:
                    got = self._fwd_unet_block(u, i, blk, params, bn, d, d_ss, skip, B, Hin, Win)
                    if got is None:
                        return None
                    rec, d, d_ss = got
                del z2
            if sv is not None:
                sv.d[f"D{i}"] = rec
            del rec, skip
            dh, dw = Hin, Win
        return d

    def _fwd_unet_block(self, u, i, blk, params, bn: BnView, d, d_ss, skip, B, Hin, Win):
        """one smp Unet decoder block over up(d) | skip -> (record for the backward when saved, output, its (scale, shift)
        when the output is conv2's raw one and the next block's conv1 applies bn2 + ReLU while staging); None: the
        recalibration pass ends with conv2's statistics of the last block"""
        last = i == len(self.spec.decoder) - 1
        y1, h1, w1, ss1 = u.conv_bn(self, blk.conv1, params, bn, d, skip, 1, B, Hin, Win, in_ss=d_ss)
        z1 = u.bn_act(self, y1, ss1, of=blk.conv1) if u.dec_z1_stored(self, blk) else None
        y2, _, _, ss2 = u.conv_bn(self, blk.conv2, params, bn, y1 if z1 is None else z1, None, 0, B, h1, w1,
                                  in_ss=ss1 if z1 is None else None)
        if last and self._recal is not None:
            return None
        if last or u.dec_out_stored(self, i):
            z2 = u.bn_act(self, y2, ss2, of=blk.conv2)    # the head kernel (or a conv1 that cannot transform) reads it
            nxt, nxt_ss = z2, None
        else:
            z2 = None
            nxt, nxt_ss = y2, ss2
        rec = dict(x=d, x_virtual=d_ss is not None, skip=skip, y1=y1, z1=z1, y2=y2, z2=z2, H=h1, W=w1) \
            if self._pass.save else None
        return rec, nxt, nxt_ss

    def _fwd_resunet_block(self, u, i, blk, params, bn: BnView, d, skip, B, Hin, Win):
        """reference network/extra/resunet/decoder.py:40-52: conv1 -> conv2 (conv-BN-ReLU each, both activations virtual)
        plus the 1x1 identity_conv (with bias) of the up-sampled + concatenated input; no activation after the sum.  The
        block output is a stored tensor (the next block and the head read it) -> (record when saved, output)"""
        y1, h1, w1, ss1 = u.conv_bn(self, blk.conv1, params, bn, d, skip, 1, B, Hin, Win)
        y2, h2, w2, ss2 = u.conv_bn(self, blk.conv2, params, bn, y1, None, 0, B, h1, w1, in_ss=ss1)
        out = u.resunet_out(self, blk, params, d, skip, y2, ss2, B, h2, w2)
        self._tr(f"D{i}.out", out)
        rec = dict(x=d, skip=skip, y1=y1, y2=y2, H=h1, W=w1) if self._pass.save else None
        return rec, out

    def _fwd_head(self, u, d, params, B, dh, dw, want_argmax: Optional[str]):
        """logits [B,K,H,W] (+ the int64 / uint8 arg-max map the head kernel writes on the way)"""
        hd, dev = self.spec.head, d.device
        K = hd.cout
        logits = torch.empty((B, K, dh, dw), dtype=torch.float32, device=dev)
        am = torch.empty((B, dh, dw), dtype=getattr(torch, want_argmax), device=dev) if want_argmax in ("int64", "uint8") \
            else None
        if self._recal is not None:
            self.recal_launches.append(("head", hd.key))
            self._recal = None
        u.head(self, d, hd.w(params), hd.bias(params), logits, am if want_argmax == "int64" else None,
               am if want_argmax == "uint8" else None, B, dh, dw, hd.cin, K)
        return logits, am

    def _forward_eval_head(self, u, x_nchw, params, bnstate, labels, lu, dist, gamma, counts, err, want_argmax):
        """eval-mode forward of the units `u` that ends in the fused evaluation head instead of the head kernel: no logits
        tensor, no int64 arg-max map -> what ``ops.head_eval`` returns"""
        from ..ops import head_eval
        d = u.decoder_output(self, x_nchw, params, bnstate)
        hd = self.spec.head
        return head_eval(d, hd.w(params).view(hd.cout, hd.k, hd.k, hd.cin), hd.bias(params), labels, lu, dist, gamma,
                         counts, err, want_argmax)
