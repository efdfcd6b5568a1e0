"""The reverse schedule of the U-Net engine, once for both precisions: the driver, the double-convolution tail every block
ends in, the three decoders reversed, the encoder loop and the max-pool + stem tail.

What differs between fp32 and bf16 comes in through ``u``, the units object of the pass (``engine_fp32.FP32_UNITS`` /
``engine_bf16.BF16_UNITS``: the unit launchers of that precision as plain functions of the engine, the activation dtype,
the ABI entry names that differ, the fusion switches, and the hooks for the stretches that are not the same sequence:
head backward, fused input gradient of a Unet block, join tail of a ResUnet block, stem weight gradient).

Tensor lifetimes are part of the schedule: every ``del`` frees a tensor before the next allocation.  A tensor a callee is
to free arrives in a container the callee empties (``dy2`` / ``dy1``: a one-element list, the dense decoder's ``G``: the
dict of node gradients), so the caller's frame holds no second reference."""
from __future__ import annotations

import torch

from .bnview import BnView


class BackwardSchedule:
    def _backward(self, u, dlogits: torch.Tensor, params: torch.Tensor, grads: torch.Tensor, saved):
        """reverse pass of the forward `saved` (default: the engine's last one) belongs to, on the units `u` (whose weight
        images the caller has prepared): writes every parameter gradient into ``grads`` (flat, laid out like ``params``) and
        calls ``grad_hook(name, lo, hi)`` as each bucket of the flat buffer completes"""
        sp, lib = self.spec, self.lib
        S = self._saved_of(saved)
        self._bwd_training = bool(S.get("training", True))
        self._bwd_enc_training = bool(S.get("enc_training", self._bwd_training))
        frozen = bool(S.get("enc_frozen", False))
        self.launches = {"dgrad": [], "wgrad": []}
        B, bn = S["B"], BnView(sp, S["bnws"])
        dev = dlogits.device

        # ---- head (fp32 in both precisions) -> gradient of the last decoder activation
        hd, h = sp.head, S["head"]
        H, W, K = h["H"], h["W"], hd.cout
        g = torch.empty_like(h["x"])
        P = lib.dt_head_bwd_rows(B, H, W)
        red = self._buf("head_red", lib.dt_head_bwd_red_floats(B, H, W, hd.cin, K), device=dev)
        u.head_bwd(self, h["x"], hd.w(params), dlogits.contiguous(), g, red, B, H, W, hd.cin, K)
        self._call("dt_head_bwd_finalize", red, P, hd.w(grads), hd.bias(grads), hd.cin, K)
        self._tr("head.g", g)

        # ---- decoder (reverse)
        skip_grads = [None] * 5  # gradient of feats[0..4] = f1..f5
        g_red = None             # BatchNorm-backward partial sums that already came with g (fused producers)
        self._head_tap_fix(grads)
        if sp.decoder_kind == "unetplusplus":
            G = {sp.decoder[-1].name: g}
            del g
            g = self._bwd_unetpp(u, S, G, params, grads, bn, B, skip_grads, dev)
            del G
        for i in (range(4, -1, -1) if sp.decoder_kind != "unetplusplus" else ()):
            if sp.decoder_kind == "resunet":
                g = self._bwd_resunet_block(u, i, sp.decoder[i], S[f"D{i}"], g, params, grads, bn, B, skip_grads)
            else:
                g, g_red = self._bwd_unet_block(u, i, S, g, g_red, params, grads, bn, B, frozen, skip_grads)
            S[f"D{i}"] = None
        self._bucket_done(sp.buckets[0])
        if frozen:      # frozen encoder weights: backward stops at the decoder (no encoder data / weight gradient)
            self._join_side()
            self.saved = None
            return

        g = [g]         # gradient wrt f5, handed over: the encoder frees it with its first block
        g, g_red = self._bwd_encoder(u, S, g, g_red, params, grads, bn, B, skip_grads)
        self._bwd_pool_stem(u, S, g, skip_grads[0], params, grads, bn, B)
        self._join_side()
        if self.grad_hook:
            self.grad_hook(*sp.buckets[4])
        self.saved = None

    # ------------------------------------------------------------------ conv2 <- BatchNorm <- conv1, every block's tail
    def _bwd_double_conv(self, u, tag, blk, rec, dy2, params, grads, bn: BnView, B, Hh, Ww, x_ss=None):
        """from the gradient of conv2's raw output (`dy2`: a one-element list, emptied here) to that of conv1's (returned):
        weight gradient of conv2 — from the stored z1, or from y1 with conv1's BatchNorm + ReLU applied while staging —,
        data gradient of conv2 with conv1's BatchNorm-backward sums in its epilogue, BatchNorm backward of conv1 (its
        activation is virtual: mask from y1 * scale + shift), weight gradient of conv1: over the up-sampled input | skip of
        a decoder record (x_ss: (scale, shift) where that input is a raw output), over the block input of an encoder one"""
        dy2 = dy2.pop()
        if rec.get("z1") is not None:
            u.wgrad(self, blk.conv2, grads, rec["z1"], None, 0, B, Hh, Ww, dy2)
        else:
            u.wgrad(self, blk.conv2, grads, rec["y1"], None, 0, B, Hh, Ww, dy2, in_ss=bn.ss(blk.conv1))
        dz1 = torch.empty_like(rec["y1"])
        if u.fuse_bn(self):
            red1 = u.dgrad_bn(self, blk.conv2, dy2, B, Hh, Ww, dz1, blk.conv1, rec["y1"], bn)
        else:
            red1 = u.dgrad(self, blk.conv2, dy2, B, Hh, Ww, dz1)
        del dy2
        self._tr(f"{tag}.dz1", dz1)
        dy1 = u.bn_bwd(self, blk.conv1, params, grads, bn, dz1, None, rec["y1"], virtual_act=True, reduced=red1)
        self._tr(f"{tag}.dy1", dy1)
        del dz1
        if "skip" in rec:
            u.wgrad(self, blk.conv1, grads, rec["x"], rec["skip"], 1, B, Hh, Ww, dy1, in_ss=x_ss)
        else:
            u.wgrad(self, blk.conv1, grads, rec["x"], None, 0, B, rec["Hin"], rec["Win"], dy1)
        return dy1

    # ------------------------------------------------------------------ the three decoders, reversed
    def _bwd_unetpp(self, u, S, G, params, grads, bn: BnView, B, skip_grads, dev):
        """reverse of the dense decoder: the blocks in reverse forward order (every consumer of a node comes before the
        node); a node's gradient is the sum over its consumers — as the up-sampled input of the block to its right
        (accumulating 2x2 sums) and as a slice of the concatenated skip of the blocks further right (accumulating slice
        copies).  G: {node name: gradient so far}, on entry the last node's (the caller lets go of it: it is freed once
        consumed).  Fills skip_grads (gradients of f1..f4) and returns the gradient of f5."""
        sp = self.spec

        def slot(name, shape):
            t = G.get(name)
            if t is None:
                t = G[name] = torch.empty(shape, dtype=u.dtype, device=dev)
                return t, 0
            return t, 1

        for blk in reversed(sp.decoder):
            tag = "P" + blk.name
            d = S[tag]
            g = G.pop(blk.name)
            self._tr(f"{tag}.g", g)
            Hh, Ww = d["H"], d["W"]
            dy2 = [u.bn_bwd(self, blk.conv2, params, grads, bn, g, None, d["y2"], virtual_act=True)]
            self._tr(f"{tag}.dy2", dy2[0])
            del g
            dy1 = self._bwd_double_conv(u, tag, blk, d, dy2, params, grads, bn, B, Hh, Ww)
            cx = blk.in_ch
            dup = torch.empty((B, Hh, Ww, cx), dtype=u.dtype, device=dev)
            dskip = None
            if d["skip"] is not None:
                dskip = torch.empty_like(d["skip"])
                u.dgrad(self, blk.conv1, dy1, B, Hh, Ww, dup, dskip, split=cx)
                self._tr(f"{tag}.dskip", dskip)
            else:
                u.dgrad(self, blk.conv1, dy1, B, Hh, Ww, dup)
            self._tr(f"{tag}.dup", dup)
            del dy1
            glow, acc = slot(blk.low, d["x"].shape)
            self._call(u.upsample_bwd_acc, dup, glow, acc, B, Hh // 2, Ww // 2, cx)
            del dup
            if dskip is not None:
                Cw = dskip.shape[-1]
                for name, (off, Cn) in zip(blk.cat, d["parts"]):
                    if len(blk.cat) == 1 and name not in G:
                        G[name] = dskip                      # the skip was the tensor itself: its gradient as is
                        continue
                    gm, acc = slot(name, (B, Hh, Ww, Cn))
                    self._call(u.channel_slice, dskip, gm, B * Hh * Ww, Cn, Cw, off, 0, acc)
            S[tag] = None
        for k in range(1, 5):
            skip_grads[4 - k] = G[f"f{k}"]      # f_k of the decoder = feats[4 - k]
            self._tr(f"Pf{k}.g", G[f"f{k}"])
        self._tr("Pf0.g", G["f0"])
        return G["f0"]

    def _bwd_resunet_block(self, u, i, blk, d, g, params, grads, bn: BnView, B, skip_grads):
        """reverse of one ResUnet decoder block, out = relu(bn2(conv2(relu(bn1(conv1(xin)))))) + identity_conv(xin) + bias:
        g = gradient of the block output -> the gradient of the block's low-resolution input; writes the skip gradient"""
        dev = g.device
        Hh, Ww = d["H"], d["W"]
        ic = blk.idc
        n_pix = B * Hh * Ww
        # identity branch: weight gradient over the virtual (up-sampled + concatenated) input, bias gradient = sum g
        u.wgrad(self, ic, grads, d["x"], d["skip"], 1, B, Hh, Ww, g)
        ws = self._buf("chsum_ws", int(getattr(self.lib, u.channel_sums + "_workspace")(n_pix, ic.cout)), device=dev)
        self._call(u.channel_sums, g, ws, n_pix, ic.cout, ic.bias(grads))
        # main branch: both activations virtual
        dy2 = [u.bn_bwd(self, blk.conv2, params, grads, bn, g, None, d["y2"], virtual_act=True)]
        self._tr(f"D{i}.dy2", dy2[0])
        dy1 = [self._bwd_double_conv(u, f"D{i}", blk, d, dy2, params, grads, bn, B, Hh, Ww)]
        return u.resunet_join(self, i, blk, d, g, dy1, B, Hh, Ww, skip_grads)

    def _bwd_unet_block(self, u, i, S, g, g_red, params, grads, bn: BnView, B, frozen, skip_grads):
        """reverse of one smp Unet decoder block: g = gradient of its (possibly virtual) output activation, g_red the
        BatchNorm-backward sums that came with it -> (gradient of the block below's activation, its sums or None)"""
        sp, lib, dev = self.spec, self.lib, g.device
        blk, d = sp.decoder[i], S[f"D{i}"]
        Hh, Ww = d["H"], d["W"]
        # the ReLU mask is recomputed from y2 * scale + shift even where z2 was stored (same arithmetic as bn_act:
        # identical mask, one tensor less to read in the reduce / apply passes)
        dy2 = [u.bn_bwd(self, blk.conv2, params, grads, bn, g, None, d["y2"], virtual_act=True, reduced=g_red)]
        self._tr(f"D{i}.dy2", dy2[0])
        x_ss = bn.ss(sp.decoder[i - 1].conv2) if d["x_virtual"] else None
        dy1 = self._bwd_double_conv(u, f"D{i}", blk, d, dy2, params, grads, bn, B, Hh, Ww, x_ss=x_ss)
        cx = blk.in_ch
        if frozen and i == 0:      # block 0's input and skip are encoder features: no data gradient at all
            return g, g_red
        # the new g is the gradient of relu(bn(y2)) of block i-1 (never stored as such; also where z2 was: the mask is
        # recomputed from y2 * scale + shift either way): that block's BatchNorm-backward sums ride in the pass that writes it
        below = (sp.decoder[i - 1].conv2, S[f"D{i - 1}"]["y2"]) if i >= 1 else None
        got = u.fused_input_grad(self, blk, below, params, bn, dy1, d, B, Hh, Ww, frozen) if i >= 1 else None
        if got is not None:      # data gradient, the up-sampling's backward and those sums in one kernel's epilogue
            g, g_red, dskip = got
            if dskip is not None:
                skip_grads[3 - i] = dskip
            self._tr(f"D{i}.dskip", dskip)
            self._tr(f"D{i}.g", g)
            return g, g_red
        dup = torch.empty((B, Hh, Ww, cx), dtype=u.dtype, device=dev)
        if d["skip"] is not None:
            # (frozen encoder: the split kernel still writes the skip's part, to a tensor nobody reads)
            dskip = torch.empty_like(d["skip"])
            u.dgrad(self, blk.conv1, dy1, B, Hh, Ww, dup, dskip, split=cx)
            skip_grads[3 - i] = None if frozen else dskip
            self._tr(f"D{i}.dskip", dskip)
        else:
            u.dgrad(self, blk.conv1, dy1, B, Hh, Ww, dup)
        self._tr(f"D{i}.dup", dup)
        del dy1
        g = torch.empty_like(d["x"])
        g_red = None
        if i >= 1 and u.fuse_bn(self):
            P = getattr(lib, u.upsample_bwd_bn + "_rows")(B, Hh // 2, Ww // 2, cx)
            red = self._buf("bn_red_up", lib.dt_bn_stats_floats(P, cx), device=dev)
            self._call(u.upsample_bwd_bn, dup, g, bn.fuse(*below), red, B, Hh // 2, Ww // 2, cx)
            g_red = (red, P)
        else:
            u.upsample_bwd(self, dup, g, B, Hh // 2, Ww // 2, cx)
        del dup
        self._tr(f"D{i}.g", g)
        return g, g_red

    # ------------------------------------------------------------------ encoder layers in reverse, max-pool, stem
    def _bwd_encoder(self, u, S, g, g_red, params, grads, bn: BnView, B, skip_grads):
        """layers 4..1 of the encoder: g = [gradient of f5] (emptied here; g_red: its BatchNorm-backward sums or None) -> the
        gradient of the max-pool output and its sums; a bucket of the flat gradient buffer completes with every layer but
        the first"""
        sp = self.spec
        g = g.pop()
        for li in (3, 2, 1, 0):
            blocks = sp.layers[li]
            for bi in range(len(blocks) - 1, -1, -1):
                blk, tag = blocks[bi], f"L{li}B{bi}"
                r = S[tag]
                Hin, Win, Hh, Ww = r["Hin"], r["Win"], r["H"], r["W"]
                # gradient buffer of the block input; a decoder skip gradient may already live there
                gin, gin_has = None, False
                if bi == 0 and li > 0 and skip_grads[li] is not None:
                    gin, gin_has = skip_grads[li], True   # block input of layer(li+1).0 is f_{li+1} = feats[li]
                if gin is None:
                    gin = torch.empty_like(r["x"])
                if blk.down is None:
                    dy2 = [u.bn_bwd(self, blk.conv2, params, grads, bn, g, r["out"], r["y2"], dres=gin, dres_acc=gin_has,
                                    reduced=g_red)]
                    gin_has = True
                    dyd = None
                    self._tr(f"{tag}.gres", gin)
                else:
                    gd = torch.empty_like(r["out"])
                    dy2 = [u.bn_bwd(self, blk.conv2, params, grads, bn, g, r["out"], r["y2"], dres=gd, reduced=g_red)]
                    dyd = u.bn_bwd(self, blk.down, params, grads, bn, gd, None, r["yd"])
                    self._tr(f"{tag}.gres", gd)
                    self._tr(f"{tag}.dyd", dyd)
                    del gd
                self._tr(f"{tag}.dy2", dy2[0])
                dy1 = self._bwd_double_conv(u, tag, blk, r, dy2, params, grads, bn, B, Hh, Ww)
                g_red = None
                if u.fuse_join(self) and bi > 0 and blk.down is None and gin_has:
                    # gin becomes the output gradient of block bi-1: this join is its last writer, so the
                    # BatchNorm-backward sums of that block's bn2 (mask: its stored output) ride along
                    rp = S[f"L{li}B{bi - 1}"]
                    g_red = u.dgrad_bn(self, blk.conv1, dy1, B, Hin, Win, gin, blocks[bi - 1].conv2, rp["y2"], bn,
                                       act=rp["out"])
                else:
                    u.dgrad(self, blk.conv1, dy1, B, Hin, Win, gin, acc=gin_has)
                gin_has = True
                del dy1
                self._tr(f"{tag}.gin1", gin)
                if dyd is not None:
                    u.wgrad(self, blk.down, grads, r["x"], None, 0, B, Hin, Win, dyd)
                    u.dgrad(self, blk.down, dyd, B, Hin, Win, gin, acc=True)
                    del dyd
                    self._tr(f"{tag}.gin", gin)
                g = gin
                S[tag] = None
            if li > 0:
                self._bucket_done(sp.buckets[4 - li])
        return g, g_red

    def _bwd_pool_stem(self, u, S, g, gf1, params, grads, bn: BnView, B):
        """max-pool backward of g, added to gf1 (the decoder's gradient of the stem activation), then the stem's BatchNorm
        backward and weight gradient"""
        sp, lib = self.spec, self.lib
        pl, stem = S["pool"], S["stem"]
        stem_red = None
        P = getattr(lib, u.maxpool_bwd_bn + "_rows")(B, pl["H"], pl["W"], 64) if u.fuse_pool(self) else 0
        if P > 0:      # even maps: the stem's BatchNorm-backward sums ride in the pass that writes its activation gradient
            red = self._buf("bn_red_pool", lib.dt_bn_stats_floats(P, 64), device=g.device)
            self._call(u.maxpool_bwd_bn, g, pl["amax"], gf1, 1, bn.fuse(sp.stem, stem["y"]), red, B, pl["H"], pl["W"], 64)
            stem_red = (red, P)
        else:
            self._call(u.maxpool_bwd, g, pl["amax"], gf1, 1, B, pl["H"], pl["W"], 64)
        self._tr("gf1", gf1)
        dy = u.bn_bwd(self, sp.stem, params, grads, bn, gf1, None, stem["y"], virtual_act=True, reduced=stem_red)
        self._tr("stem.dy", dy)
        u.stem_wgrad(self, stem, dy, grads, B)
