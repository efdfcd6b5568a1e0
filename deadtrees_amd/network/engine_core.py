"""What both precisions of the U-Net engine share: the library handle and the ONE launch path, the workspaces, the
profiling bracket, the weight tables and weight-image caches, the weight-gradient side stream and the fp32 BatchNorm
coefficient launches, the per-pass record of the BatchNorm mode.  The unit launchers live in ``engine_fp32`` /
``engine_bf16``, the two schedules in ``engine_forward`` / ``engine_backward``; ``engine.UNetEngine`` mixes them in."""
from __future__ import annotations

import contextlib
import os

import ctypes as C
from typing import Callable, Optional

import torch

from .. import _lib
from .._lib import stream as _stream
from .bnview import BnView
from .spec import ConvSpec, UNetSpec

BN_EPS = 1e-5
BN_MOMENTUM = 0.1


def _arg(a):
    """python value -> ABI argument: tensors travel as device addresses, structures by reference"""
    if isinstance(a, torch.Tensor):
        return a.data_ptr()
    if isinstance(a, C.Structure):
        return C.byref(a)
    return a


def _pair(ss):
    """an optional (scale, shift) pair as two pointer arguments"""
    return ss if ss else (None, None)


class _Saved:
    """activations kept from forward for the hand-written backward"""
    __slots__ = ("d",)

    def __init__(self):
        self.d = {}


class _Pass:
    """the forward pass in flight (set by ``engine_forward._forward``, read by the units of either precision): the
    BatchNorm mode — decoder / encoder layers on batch statistics, else on their running statistics —, what is kept for a
    backward (`save`; of the encoder only `enc_save`: not with frozen weights), and where the fp32 inference forms with
    BatchNorm + ReLU in the convolution's epilogue run (set from the units' ``fuse_eval`` rule)"""
    __slots__ = ("dec_batch", "enc_batch", "save", "enc_save", "enc_frozen", "fuse_enc", "fuse_dec")

    def __init__(self, dec_batch=False, enc_batch=False, save=False, enc_save=False, enc_frozen=False):
        self.dec_batch, self.enc_batch, self.save, self.enc_save = bool(dec_batch), bool(enc_batch), bool(save), bool(enc_save)
        self.enc_frozen, self.fuse_enc, self.fuse_dec = bool(enc_frozen), False, False


class EngineCore:
    def __init__(self, spec: UNetSpec):
        self.spec = spec
        self.lib = _lib.load()
        self._ws = {}
        self._tables = {}             # per-device weight tables (_wino_table, _weight_table)
        self.saved: Optional[_Saved] = None
        self.grad_hook: Optional[Callable[[str, int, int], None]] = None
        # when a list: every dt_conv2d launch appends (kernel name, algorithmic FLOPs, start, end events)
        self.profile: Optional[list] = None
        self._weights_epoch = 0
        self._bn_epoch = 0            # bumped by every training-mode forward (running statistics written on the device)
        self._affine_fresh = False
        self._u_all = self._ud_all = None     # Winograd weight images of the current forward / backward pass
        # Weight gradients on a side stream, concurrent with the data-gradient / BatchNorm chain.  Round 1 (direct
        # kernels, 2 workgroups per CU): SLOWER (485 vs 528 tiles/s fp32, 1505 vs 1566 bf16) — co-resident wgrad / dgrad
        # workgroups halve each other's occupancy and share the matrix pipe.  Round 2, fp32 Winograd path: the kernels
        # own a whole CU (148 KB LDS, 512 registers per lane), nothing co-resides, and the second stream only fills
        # the launch gaps and tails of the ~200 short kernels of the backward pass: 716.6 vs 701.6 tiles/s on one box.
        # fp32: on with the Winograd kernels (DT_OVERLAP_WGRAD=0/1 overrides); bf16: off.
        self.overlap_wgrad = os.environ.get("DT_OVERLAP_WGRAD", "1" if os.environ.get("DT_FP32_WINOGRAD", "1") != "0" else "0") != "0"
        self.overlap_wgrad_bf16 = bool(os.environ.get("DT_OVERLAP_WGRAD_BF16"))
        self._bwd_training = True
        self._bwd_enc_training = True
        # encoder = stem + layers 1-4: the first convolutions of the spec, the contiguous range [0, encoder_hi) of the flat
        # buffer (the head+decoder bucket starts there)
        self._enc_index = {c.index for c in spec.convs if c.key.startswith("encoder.")}
        self.encoder_hi = spec.buckets[0][1]
        # per backward: the convolutions whose data gradient / weight gradient were launched (tests, timing labels)
        self.launches = {"dgrad": [], "wgrad": []}
        # BatchNorm recalibration forward (stochastic weight averaging): the device momentum float[1] every
        # dt_bn_finalize_dev of the current pass reads (None outside such a pass), and the launch record of the last one:
        # ("conv" | "bn_finalize_dev" | "bn_act" | "head", convolution key)
        self._recal: Optional[torch.Tensor] = None
        self.recal_launches: list = []
        # BatchNorm-backward reduction of a block-output layer inside the fp32 gradient-JOIN epilogue: measured slower
        # than the separate pass (526 vs 530 tiles/s, same box: 48 extra loads per lane in the read-modify-write
        # epilogue); the bf16 path keeps it (its join epilogue is LDS-staged, +0.5 %).  Kernel support stays tested.
        # Round 3, Winograd engine: the join epilogue form 3 of conv3x3_wino_kernel carries the sums at +0.7 % of the step
        # (763.9 vs 758.8 tiles/s, same box) and removes 13 of the 23 remaining bn_bwd_reduce passes: on with Winograd.
        self.fuse_join_fp32 = os.environ.get("DT_FUSE_JOIN_FP32", "1" if os.environ.get("DT_FP32_WINOGRAD", "1") != "0" else "0") != "0"
        self._fuse_bn = not os.environ.get("DT_NO_BN_FUSE")   # A/B switch for the plain fused reductions
        # fp32 3x3 stride-1 layers (forward + data gradient) on the Winograd F(2x2,3x3) kernel where its shape conditions
        # hold (conv_wino.hip: 1.6-2.0x the direct kernel per layer); DT_FP32_WINOGRAD=0 keeps the exact-fma direct kernel
        self.winograd = os.environ.get("DT_FP32_WINOGRAD", "1") != "0"
        # conv1 activations of the blocks whose conv2 runs on the Winograd kernels are materialised (bn_act) instead of
        # being applied while conv2 / its weight gradient stage their input: the fused form costs those kernels 11-13 %
        # (one wave per SIMD: the staging instructions are not free behind the MFMAs), the extra pass 0.4 ms — measured 713 vs 704
        # tiles/s; DT_MATERIALIZE_Z1=0 restores the fused form (a gain with the direct kernels: +2 % in round 1)
        # inference (eval mode, nothing saved): BatchNorm + ReLU (+ residual) in the Winograd epilogue, DT_FUSE_EVAL=0 = A/B
        self._fuse_eval_opt = os.environ.get("DT_FUSE_EVAL", "1") != "0"
        self._bf16_images_fused = os.environ.get("DT_BF16_IMAGES_FUSED", "1") != "0"   # four bf16 weight images in one launch
        self._fuse_pool_bn = os.environ.get("DT_FUSE_POOL_BN", "1") != "0"   # stem BatchNorm-backward sums in the max-pool backward
        self._pass = _Pass()
        self._mat_z1 = os.environ.get("DT_MATERIALIZE_Z1", "1" if self.winograd else "0") != "0"
        # the same for the decoder block outputs that feed a Winograd conv1 (716.6 vs 712.8 tiles/s)
        self._mat_z2 = os.environ.get("DT_MATERIALIZE_Z2", "1" if self.winograd else "0") != "0"
        # bf16: the input-transforming form of the LDS-DMA kernel stages its input through registers (no DMA); a stored
        # bf16 activation (2 + 2 B per element) lets conv2 and its weight gradient run the pure-DMA form: 2,235 vs 2,203
        self._mat_z1_bf16 = os.environ.get("DT_BF16_MAT_Z1", "1") != "0"
        self._mat_dec_bf16 = os.environ.get("DT_BF16_MAT_DEC", "1") != "0"
        # when a dict: the training pass of either precision (fp32: forward / backward, bf16: forward_bf16_train /
        # backward_bf16) stores a copy of every intermediate tensor it produces and does not keep for the backward anyway,
        # under the names of oracle/unet_bf16_ref.py (teacher-forced parity tests); None in production — then the pass
        # launches and allocates nothing for it.  Not under graph capture (the copies are allocations of the pass).
        self.trace: Optional[dict] = None

    # ------------------------------------------------------------------ the launch path
    def _call(self, name: str, *args):
        """one ABI call on the current stream: tensors -> pointers, structures by reference, the stream appended, the
        return code checked under the entry point's name"""
        rc = getattr(self.lib, name)(*[_arg(a) for a in args], _stream())
        if rc != 0:
            _lib.check(rc, name)

    def _rows(self, name: str, *args) -> int:
        """a host-side query of the ABI that answers with a positive row / byte count (0 or less: an error)"""
        n = getattr(self.lib, name)(*[_arg(a) for a in args])
        if n <= 0:
            raise RuntimeError(f"{name}: {self.lib.dt_last_error().decode()}")
        return n

    # ------------------------------------------------------------------ helpers
    def _tr(self, name: str, t: Optional[torch.Tensor]):
        if self.trace is not None and t is not None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("engine.trace is for eager passes: set it to None before capturing a graph")
            self.trace[name] = t.clone()

    def _buf(self, name: str, numel: int, dtype=torch.float32, device=None) -> torch.Tensor:
        t = self._ws.get(name)
        if t is None or t.numel() < numel or t.device != device:
            t = torch.empty(max(numel, 1), dtype=dtype, device=device)
            self._ws[name] = t
        return t

    @contextlib.contextmanager
    def capture_workspaces(self, keep=()):
        """graph capture: the workspaces the captured pass allocates live (and stay) in the graph's pool.  Installs a
        fresh ``_ws`` — with the eager entries whose name starts with one of `keep` — and yields it: the caller keeps
        that dict alive next to its graph.  The eager workspaces come back on exit."""
        eager = self._ws
        self._ws = {k: v for k, v in eager.items() if k.startswith(tuple(keep))} if keep else {}
        try:
            yield self._ws
        finally:
            self._ws = eager

    def _const_vec(self, value: float, n: int, device) -> torch.Tensor:
        key = f"const_{value}"
        t = self._ws.get(key)
        if t is None or t.numel() < n or t.device != device:
            t = torch.full((max(n, 512),), float(value), dtype=torch.float32, device=device)
            self._ws[key] = t
        return t[:n]

    def _cat_channels(self, tensors):
        """torch.cat(dim=1) of NHWC activations through dt_channel_slice -> (wide tensor, [(channel offset, width)])"""
        if len(tensors) == 1:
            return tensors[0], [(0, tensors[0].shape[-1])]
        B, H, W = tensors[0].shape[:3]
        Cw = sum(t.shape[-1] for t in tensors)
        bf = tensors[0].dtype == torch.bfloat16
        wide = torch.empty((B, H, W, Cw), dtype=tensors[0].dtype, device=tensors[0].device)
        parts, off = [], 0
        for t in tensors:
            Cn = t.shape[-1]
            self._call("dt_channel_slice_bf16" if bf else "dt_channel_slice", t, wide, B * H * W, Cn, Cw, off, 1, 0)
            parts.append((off, Cn))
            off += Cn
        return wide, parts

    # ---- per-launch profiling (bench.py's roofline table): `self.profile` is None in production; as a list it receives
    # (kernel / family name, algorithmic FLOPs, start event, end event, algorithmic HBM bytes) per bracketed launch group
    def _pb(self):
        if self.profile is None:
            return None
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
        return e0

    def _pe(self, e0, name: str, flops: float, nbytes: float):
        if e0 is None:
            return
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        self.profile.append((name, float(flops), e0, e1, float(nbytes)))

    def _conv_work(self, desc, elt: int = 4, extra_bytes: float = 0.0):
        """(algorithmic FLOPs, algorithmic HBM bytes) of a convolution / its weight gradient described by `desc`:
        2 k^2 Cin Cout per output pixel; stored input(s) once (an upsampled source at its stored size) + output once
        (+ the read of a read-modify-write join) + weights once (+ what the caller's epilogue moves on top).
        elt: bytes per activation / weight element.  The bf16 space-to-depth stem (the only 4x4 window) counts the
        7x7 x in_channels window it stands for."""
        flops = 2.0 * desc.ksize ** 2 * (desc.C0 + desc.C1) * desc.Cout * desc.Ho * desc.Wo * desc.B
        if desc.mode0 == 2:
            flops /= 4.0   # transposed conv: 3/4 of the zero-inserted input does no algorithmic work
        if elt == 2 and desc.ksize == 4:
            flops = 2.0 * 49 * self.spec.in_channels * desc.Cout * desc.Ho * desc.Wo * desc.B
        sdiv = 4 if desc.mode0 else 1
        nbytes = elt * desc.B * (desc.Hin * desc.Win * (desc.C0 / sdiv + desc.C1) +
                                 desc.Ho * desc.Wo * desc.Cout * (2 if desc.accumulate else 1)) + \
            elt * desc.ksize ** 2 * (desc.C0 + desc.C1) * desc.Cout
        return flops, nbytes + extra_bytes

    def _desc(self, B, Hin, Win, C0, C1, mode0, Ho, Wo, Cout, k, stride, pad, split=0, acc=0):
        return _lib.ConvDesc(B, Hin, Win, C0, C1, mode0, Ho, Wo, Cout, k, stride, pad, split, acc)

    def _conv_desc(self, c: ConvSpec, src0, src1, mode0, B, Hin, Win):
        """descriptor of the forward convolution c over src0 (| src1) at the logical input size Hin x Win"""
        C0 = src0.shape[-1]
        C1 = 0 if src1 is None else src1.shape[-1]
        assert C0 + C1 == c.cin, (c.key, C0, C1, c.cin)
        return self._desc(B, Hin, Win, C0, C1, mode0, c.out_size(Hin), c.out_size(Win), c.cout, c.k, c.stride, c.pad)

    # ------------------------------------------------------------------ BatchNorm coefficients (fp32 in both precisions)
    def _batch_stats(self, c: ConvSpec) -> bool:
        """the ONE rule for the BatchNorm mode of a layer in the forward pass in flight: batch statistics (True) or its
        running statistics, by whether the layer belongs to the encoder"""
        p = self._pass
        return p.enc_batch if c.index in self._enc_index else p.dec_batch

    def _bn_eval_affine(self, c: ConvSpec, params, bn: BnView):
        """(scale, shift) of conv c from its running statistics; skipped while the coefficients of the previous
        inference call are still valid (`_affine_fresh`, see forward).  A convolution bias in front of the BatchNorm
        (EfficientUnet++ blocks) is folded into the shift: shift + scale * bias"""
        if not self._affine_fresh and c.has_cbias:
            self._call("dt_bn_eval_affine_bias", c.gamma(params), c.beta(params), bn.running_mean(c), bn.running_var(c),
                       c.conv_bias(params), BN_EPS, c.cout, bn.scale(c), bn.shift(c))
        elif not self._affine_fresh:
            self._call("dt_bn_eval_affine", c.gamma(params), c.beta(params), bn.running_mean(c), bn.running_var(c),
                       BN_EPS, c.cout, bn.scale(c), bn.shift(c))
        return bn.ss(c)

    def _bn_finalize(self, c: ConvSpec, params, bn: BnView, stats, P: int, count: int):
        """batch statistics of conv c (P partial rows in `stats` over `count` pixels) -> mean / invstd / scale / shift, and
        into the running statistics with the momentum constant — or, in a recalibration pass, with the cumulative-average
        momentum read from the device"""
        if self._recal is not None:
            self._call("dt_bn_finalize_dev", stats, P, c.cout, float(count), c.gamma(params), c.beta(params), BN_EPS,
                       self._recal, bn.running_mean(c), bn.running_var(c), bn.mean(c), bn.invstd(c), bn.scale(c),
                       bn.shift(c))
            self.recal_launches += [("conv", c.key), ("bn_finalize_dev", c.key)]
        else:
            self._call("dt_bn_finalize", stats, P, c.cout, float(count), c.gamma(params), c.beta(params), BN_EPS,
                       BN_MOMENTUM, bn.running_mean(c), bn.running_var(c), bn.mean(c), bn.invstd(c), bn.scale(c),
                       bn.shift(c))
        return bn.ss(c)

    def _bn_eval_stats(self, c: ConvSpec, bn: BnView):
        """a backward pass may follow an eval-mode layer (frozen-BatchNorm fine-tuning): xhat uses the running stats"""
        self._call("dt_bn_eval_stats", bn.running_mean(c), bn.running_var(c), BN_EPS, c.cout, bn.mean(c), bn.invstd(c))

    def _rec_act(self, c: Optional[ConvSpec]):
        """recalibration launch record: the normalise pass of convolution c"""
        if self._recal is not None:
            self.recal_launches.append(("bn_act", None if c is None else c.key))

    # ------------------------------------------------------------------ Winograd weight images (conv_wino.hip)
    def _wino_table(self, device, dgrad: bool):
        """(device table, rows, blocks, total floats, {conv key: offset}) of the layers whose forward conv (dgrad False)
        or stride-1 data gradient (dgrad True: Cin / Cout swapped, read from the dt_weight_images mode-0 buffer) can run
        on the Winograd kernel: 3x3 stride 1 pad 1, input channels a multiple of 16, output channels a multiple of 64"""
        key = ("wino", bool(dgrad), str(device))
        tab = self._tables.get(key)
        if tab is None:
            rows, blocks, off, offs = [], 0, 0, {}
            for c in self.spec.convs:
                if c is self.spec.stem or c is self.spec.head or c.k != 3 or c.stride != 1 or c.pad != 1 or c.depthwise:
                    continue
                cin, cout = (c.cout, c.cin) if dgrad else (c.cin, c.cout)
                if cin % 16 or cout % 64:
                    continue
                rows.append([c.w_off, off, cin, cout, blocks])
                offs[c.key] = (off, 16 * cin * cout)
                blocks += ((cout + 63) // 64) * ((cin // 4 + 3) // 4)
                off += 16 * cin * cout
            tab = (torch.tensor(rows, dtype=torch.int32).to(device) if rows else None, len(rows), blocks, off, offs)
            self._tables[key] = tab
        return tab

    def _wino_images(self, weights: torch.Tensor, name: str, dgrad: bool):
        tab, n, blocks, total, _ = self._wino_table(weights.device, dgrad)
        if n == 0:
            return None
        buf = self._buf(name, total, device=weights.device)
        self._call("dt_winograd_weight_images", weights, buf, tab, n, blocks)
        return buf

    def _wino_fwd_weights(self, params: torch.Tensor):
        """forward images of every eligible layer, rebuilt when the flat parameter buffer changed (one launch)"""
        if not self.winograd:
            return None
        key = (params.data_ptr(), params._version, self._weights_epoch)
        if self._ws.get("wino_u_key") != key:
            self._ws["wino_u_val"] = self._wino_images(params, "wino_u", False)
            self._ws["wino_u_key"] = key
        return self._ws["wino_u_val"]

    def _u(self, c: ConvSpec, dgrad: bool = False):
        """the Winograd image of conv c (forward / data gradient) or None"""
        buf = self._ud_all if dgrad else self._u_all
        if buf is None:
            return None
        ent = self._wino_table(buf.device, dgrad)[4].get(c.key)
        return None if ent is None else buf[ent[0]:ent[0] + ent[1]]

    # ------------------------------------------------------------------ per-layer weight images (flipped fp32, bf16)
    def _weight_table(self, device):
        """device table of the BatchNorm-ed convolutions except the stem for dt_weight_images:
        (w_off, taps, Cin, Cout, first_tile) rows, built once per device"""
        key = ("wtab", str(device))
        tab = self._tables.get(key)
        if tab is None:
            rows, tiles = [], 0
            for c in self.spec.convs:
                if c is self.spec.stem or c is self.spec.head:
                    continue
                rows.append([c.w_off, c.k * c.k, c.cin, c.cout, tiles])
                tiles += c.k * c.k * ((c.cin + 31) // 32) * ((c.cout + 31) // 32)
            tab = (torch.tensor(rows, dtype=torch.int32).to(device), len(rows), tiles)
            self._tables[key] = tab
        return tab

    def _weight_images(self, params: torch.Tensor, out: torch.Tensor, mode: int):
        tab, n, tiles = self._weight_table(params.device)
        self._call("dt_weight_images", params, out, tab, n, tiles, mode)

    def _bf16_weights(self, params: torch.Tensor, dgrad: bool = False, chunked: bool = False):
        """bf16 images of every conv weight except stem and head: [tap][Cout][Cin] for the forward convs, or the
        data-gradient image (HWIO with reversed taps).  Repacked when the flat parameter buffer changed: torch's
        version counter catches torch-side writes, ``self.weights_dirty`` the fused optimiser's raw writes."""
        name = ("bf16_wd" if dgrad else "bf16_w") + ("c" if chunked else "")   # chunked: [tap][K/32][N][32] (DMA kernels)
        key = (params.data_ptr(), params._version, self._weights_epoch)
        if self._ws.get(name + "_key") == key:
            return self._ws[name]
        buf = self._ws.get(name)
        if buf is None or buf.device != params.device:
            buf = torch.empty(self.spec.n_params, dtype=torch.bfloat16, device=params.device)
        mode = (4 if dgrad else 3) if chunked else (2 if dgrad else 1)
        self._weight_images(params, buf, mode)     # every layer's image in one launch
        self._ws[name + "_key"], self._ws[name] = key, buf
        return buf

    def _bf16_weights_all(self, params: torch.Tensor):
        """the four bf16 images a training step reads (forward / data gradient, plain / chunked) in ONE launch — one read of
        the fp32 parameters instead of four; fills the caches _bf16_weights() looks at"""
        key = (params.data_ptr(), params._version, self._weights_epoch)
        names = ("bf16_w", "bf16_wd", "bf16_wc", "bf16_wdc")
        if all(self._ws.get(n + "_key") == key for n in names):
            return
        bufs = []
        for n in names:
            b = self._ws.get(n)
            if b is None or b.device != params.device:
                b = torch.empty(self.spec.n_params, dtype=torch.bfloat16, device=params.device)
            bufs.append(b)
        tab, nl, tiles = self._weight_table(params.device)
        self._call("dt_weight_images_bf16_all", params, *bufs, tab, nl, tiles)
        for n, b in zip(names, bufs):
            self._ws[n + "_key"], self._ws[n] = key, b

    def mark_weights_changed(self):
        """call after writing the flat parameter buffer behind torch's back (fused optimiser step)"""
        self._weights_epoch += 1

    # ---- weight gradients run on a side stream, concurrently with the data-gradient chain of the main stream:
    # both only depend on dy, and the many tiny reduction / finalize launches of either chain otherwise leave
    # the chip idle.  Ordering: side waits for the event recorded after dy was produced; main waits for the side
    # stream before a gradient bucket is handed to the reducer / optimiser.  Tensors touched by the side stream are
    # registered with the caching allocator (record_stream) so they are not recycled while still in use.
    def _side_stream(self, device):
        st = self._ws.get("side_stream")
        if st is None or st.device != device:
            # high priority = its own hardware queue.  ROCm deals streams round-robin onto GPU_MAX_HW_QUEUES (4) hardware
            # queues; once an RCCL process group has created its streams a default-priority side stream lands on the
            # queue of the main stream and the weight gradients serialise behind the chain they should run beside
            # (measured with an RCCL group initialised, same box: 729 tiles/s -> 770; without a group 767 either way)
            st = torch.cuda.Stream(device=device, priority=int(os.environ.get("DT_SIDE_PRIORITY", "-1")))
            self._ws["side_stream"] = st
        return st

    def _on_side(self, fn, *tensors):
        main = torch.cuda.current_stream()
        side = self._side_stream(main.device)
        ev = torch.cuda.Event()
        ev.record(main)
        side.wait_event(ev)
        for t in tensors:
            if t is not None:
                t.record_stream(side)
        with torch.cuda.stream(side):
            fn()

    def _join_side(self):
        main = torch.cuda.current_stream()
        side = self._ws.get("side_stream")
        if side is not None:
            ev = torch.cuda.Event()
            ev.record(side)
            main.wait_event(ev)

    def _bucket_done(self, bucket):
        """a contiguous range of the flat gradient buffer is complete: hand it to ``grad_hook`` (the data-parallel
        all-reduce).  Its producers ran on the main stream (BatchNorm / head gradients) AND on the weight-gradient side
        stream; instead of joining main <- side (which drains the overlap at every bucket) the hook is called with the
        SIDE stream current, after that stream has been ordered behind main's work so far: the collective waits for
        both, the main stream waits for nobody."""
        if not self.grad_hook:
            return
        main = torch.cuda.current_stream()
        side = self._ws.get("side_stream")
        if side is None:
            self.grad_hook(*bucket)
            return
        ev = torch.cuda.Event()
        ev.record(main)
        side.wait_event(ev)
        with torch.cuda.stream(side):
            self.grad_hook(*bucket)

    def _saved_of(self, saved: Optional[_Saved]) -> dict:
        sv = saved if saved is not None else self.saved
        if sv is None:
            raise RuntimeError("backward called without a saved forward (was another forward run in between?)")
        return sv.d

    def _head_tap_fix(self, grads):
        """ResUnet: the 1x1 head lives in the centre tap of the 3x3 head kernel: the other taps' gradients stay zero"""
        hd = self.spec.head
        if self.spec.decoder_kind == "resunet" and hd.sd_k == 1:
            gw = hd.w(grads).view(hd.cout, 9, hd.cin)
            gw[:, :4].zero_()
            gw[:, 5:].zero_()
