"""One data-parallel training step of the reference recipe on the HIP path.

What Lightning does around ``SemSegment.training_step`` in the reference (deadtrees/train.py:113 with
configs/trainer/default.yaml): forward -> loss -> ``loss.backward()`` -> ``clip_grad_norm_(0.5)`` ->
``Adam.step()``.  Here the same sequence runs on the hand-written kernels with one flat gradient
buffer; with ``world_size > 1`` (one process per GPU) the gradient buckets are all-reduced (sum) over
RCCL/xGMI as soon as backward has produced them, overlapped with the rest of backward; the 1/N of the
mean is folded into the optimiser's clip coefficient (Lightning-DDP semantics: per-replica BatchNorm
statistics, mean-reduced gradients — SURVEY §8e).
"""
from __future__ import annotations

import hashlib
import json
import math
import os
from dataclasses import dataclass
from functools import partial
from typing import Callable, List, Optional, Sequence

import torch

from .data.distmap import distmaps_on_device
from .loss.seg_loss import PART_KEYS, loss_algebra, loss_backward, loss_forward
from .network.unet import UNetHIP
from .ops import FlatAdam, WeightAverager, confusion_matrix, eval_accumulate, object_histogram, prob_histogram
from .utils.graph_replay import GraphReplay, ReplayCache


class GradReducer:
    """Bucketed asynchronous all-reduce of ranges of the flat gradient buffer."""

    def __init__(self, group=None):
        import torch.distributed as dist
        self.dist = dist
        self.group = group
        self.world = dist.get_world_size(group)
        self.pending: List = []
        self.grads: Optional[torch.Tensor] = None

    def attach(self, grads: torch.Tensor):
        self.grads = grads

    def hook(self, name: str, lo: int, hi: int):
        if self.world == 1:
            return
        view = self.grads[lo:hi]
        self.pending.append(self.dist.all_reduce(view, op=self.dist.ReduceOp.SUM, group=self.group, async_op=True))

    def wait(self):
        for w in self.pending:
            w.wait()
        self.pending.clear()


class HipTrainer:
    def __init__(self, model: UNetHIP, lr: float = 3e-4, clip: float = 0.5,
                 losses: Sequence[str] = ("GDICE", "FOCAL"), distributed: bool = False, group=None,
                 precision: str = "fp32", graph: bool = False, average=None):
        """average: None | "swa" | ("ema", decay) — an averaged copy of the flat parameters (``self.averager``,
        torch.optim.swa_utils.AveragedModel semantics).  "ema": updated by every step right after Adam, inside the
        captured graph, and left alone by a skipped (non-finite) step.  "swa": updated by ``update_average()``, which
        ``fit(swa=...)`` calls once per epoch.  None allocates nothing and adds no launch.  With distributed=True the
        average is local to each rank: ranks hold equal parameters, hence equal averages, and no collective runs.
        graph=True: after two eager steps the whole step (forward, loss, backward, clip, Adam) is captured into a
        HIP graph and replayed — ~750 kernel launches become one, which matters once the bf16 step is shorter than
        the Python launch path.  Warm-up, capture and replay are ``utils.graph_replay``'s."""
        if getattr(model, "inference_only", False):
            model._require_trainable("HipTrainer (missing backward path)")
        if not model.flat_params.is_cuda:
            raise RuntimeError("HipTrainer needs the model on an MI355X (model.to('cuda'))")
        self.model = model
        model.deliver_grad_to_autograd = False   # this trainer reads the engine's flat gradient buffer itself
        if precision not in ("fp32", "bf16"):
            raise ValueError(f"precision {precision!r}: use 'fp32' or 'bf16'")
        model.precision = precision
        self.losses = tuple(losses)
        self.opt = FlatAdam(model.flat_params.data, lr=lr, max_norm=clip)
        self.reducer = GradReducer(group) if distributed else None
        self.world = self.reducer.world if self.reducer else 1
        if self.reducer:
            self.reducer.attach(model._grad_buffer())
            model.engine.grad_hook = self.reducer.hook
        self.last = {}
        # with distributed=True the bucketed RCCL all-reduces are captured too (rehearsed at world size 1 on RCCL 2.26;
        # bench.py keeps multi-GPU runs eager until that has run on a real 8-GPU node)
        self.use_graph = bool(graph)
        self._step_replays = ReplayCache(keep_all=False)    # new shapes / loss blend: drop the old graph, warm up again
        self.averager = None if average is None else WeightAverager(model.flat_params.data, average)
        self._recal_replays = ReplayCache(keep_all=False)
        self._val_replays = ReplayCache(keep_all=True)      # one captured graph per key (shapes, precision, loss set)
        self._val_state = None           # device accumulators of a validation epoch (the captured graphs write them)
        self._obj_state = None           # those of validate(objects=...): allocated on first use, untouched without it

    @torch.no_grad()
    def broadcast_parameters(self, src: int = 0):
        if self.reducer and self.world > 1:
            self.reducer.dist.broadcast(self.model.flat_params.data, src, group=self.reducer.group)
            self.reducer.dist.broadcast(self.model.bn_state, src, group=self.reducer.group)

    # ------------------------------------------------------------------ weight averaging
    def _need_averager(self, what: str) -> WeightAverager:
        if self.averager is None:
            raise RuntimeError(f"{what}: this trainer keeps no average (HipTrainer(average='swa' | ('ema', decay)))")
        if self.averager.p.data_ptr() != self.model.flat_params.data_ptr():
            self.averager.to(self.model.flat_params.data)      # the model moved (model.to(device)): follow it
        return self.averager

    def update_average(self):
        """fold the current parameters into the average (once per epoch under SWA; an EMA is updated by ``step``)"""
        self._need_averager("update_average").update()

    @torch.no_grad()
    def swap_in_average(self):
        """the averaged weights become the model's parameters.  The engine's weight images (Winograd, bf16) are marked
        stale; Adam's moments stay as they are.  The running BatchNorm statistics still belong to the old weights:
        ``update_bn`` recomputes them."""
        self._need_averager("swap_in_average").copy_to(self.model.flat_params.data)
        self.model.engine.mark_weights_changed()

    @torch.no_grad()
    def update_bn(self, loader, to_device=None) -> int:
        """``UNetHIP.update_bn`` in this trainer's precision; with graph=True the statistics-only forward (the device
        batch count and momentum included) is captured after two eager batches and replayed, one graph per input shape.
        Distributed: every rank recalibrates on its own batches, then rank 0's statistics are broadcast."""
        m = self.model
        k = m.update_bn(loader, precision=m.precision, to_device=to_device,
                        _run=self._recal_graph_batch if self.use_graph else None)
        if self.reducer and self.world > 1:
            self.reducer.dist.broadcast(m.bn_state, 0, group=self.reducer.group)
        return k

    def _recal_graph_batch(self, x: torch.Tensor, precision: str):
        """``recalibrate_batch`` through ``GraphReplay``: two eager batches, then one graph per (shape, precision)"""
        m = self.model
        self._recal_replays.get((tuple(x.shape), precision), lambda: GraphReplay(
            m.engine, lambda x: m.recalibrate_batch(x, precision), warmup=2))(x)

    # ------------------------------------------------------------------ validation epoch
    def _val_buffers(self):
        """the device accumulators of a validation epoch: epoch f64[9] (weighted sums of the eight ``parts`` + the sum of
        weights), confusion counts int64 [2,K,K], label flag int32[1], and "hist", the probability histogram int64
        [2,K,2,256] of ``validate(curves=True)`` (``loss/curves.py``).  Allocated once: captured graphs write them."""
        dev, K = self.model.flat_params.device, self.model.spec.classes
        st = self._val_state
        if st is None or st["epoch"].device != dev:
            st = self._val_state = {"epoch": torch.zeros(9, dtype=torch.float64, device=dev),
                                    "counts": torch.zeros((2, K, K), dtype=torch.int64, device=dev),
                                    "err": torch.zeros(1, dtype=torch.int32, device=dev),
                                    "hist": torch.zeros((2, K, 2, 256), dtype=torch.int64, device=dev)}
            self._val_replays.clear()
        return st

    def _obj_buffers(self):
        """the accumulators of ``validate(objects=...)`` (``loss/objects.py``): "hist" int64 [K,2,256,256] and "targets"
        int64 [K].  Kept apart from ``_val_buffers``: an epoch without ``objects`` neither allocates nor zeroes them."""
        dev, K = self.model.flat_params.device, self.model.spec.classes
        st = self._obj_state
        if st is None or st["hist"].device != dev:
            st = self._obj_state = {"hist": torch.zeros((K, 2, 256, 256), dtype=torch.int64, device=dev),
                                    "targets": torch.zeros(K, dtype=torch.int64, device=dev)}
        return st

    def _val_batch(self, img, mask, lu, distmap, alpha, curves=False, objects=None):
        """one validation batch, launches only: eval-mode forward up to the decoder output, the fused evaluation head
        (losses with GWDICE: logits, ``loss_forward`` and ``confusion_matrix``, the unfused chain), the scalar algebra
        and the weighted accumulation into the epoch buffers.  Reads no module mode and writes no model state.
        ``curves``: the unfused chain as well, plus ONE ``prob_histogram`` of the logits into the epoch's histogram — the
        fused ``dt_head_eval`` never materialises the logits, so it has nothing a histogram could read.  ``objects`` (an
        ``ObjectSweep``): the unfused chain too; ``q`` is ``prob_histogram``'s own (into the epoch's histogram with ``curves``,
        into a throw-away one without), and ``object_histogram`` adds the batch's crowns to the object buffers."""
        m, eng, st = self.model, self.model.engine, self._val_buffers()
        params = m.flat_params.detach()
        B, K = img.shape[0], m.spec.classes
        H, W = img.shape[2], img.shape[3]
        x = img if img.dtype == torch.float32 else img.float()
        boundary = any(n.startswith("BOUNDARY") for n in self.losses)
        if boundary and distmap is None:
            distmap = distmaps_on_device(mask, K)
        dist = distmap if boundary else None
        if "GWDICE" in self.losses or curves or objects is not None:
            if m.precision == "bf16":
                logits, am = eng.forward_bf16_eval(x, params, m.bn_state, want_argmax="uint8")
            else:
                logits, am = eng.forward(x, params, m.bn_state, False, save=False, want_argmax="uint8")
            parts, err, _ = loss_forward(logits, mask, dist, {"losses": self.losses, "alpha": alpha})
            _, err_cm = confusion_matrix(am, mask, lu, K=K, counts=st["counts"])
            torch.maximum(st["err"], torch.maximum(err, err_cm), out=st["err"])
            if objects is not None:
                ost = self._obj_buffers()
                if curves:
                    _, _, q = prob_histogram(logits, mask, lu, hist=st["hist"], err=st["err"], logits=True, want_q=True)
                else:
                    _, _, q = prob_histogram(logits, mask, None, err=st["err"], logits=True, want_q=True)
                object_histogram(q, mask.contiguous(), objects, hist=ost["hist"], targets=ost["targets"], err=st["err"])
            elif curves:
                prob_histogram(logits, mask, lu, hist=st["hist"], err=st["err"], logits=True)
        else:
            head = eng.forward_bf16_eval_head if m.precision == "bf16" else eng.forward_eval_head
            acc, _, _, _ = head(x, params, m.bn_state, mask, lu, dist, 2.0, st["counts"], st["err"])
            parts = loss_algebra(acc, self.losses, B, K, H, W, dist is not None, alpha)[0]
        eval_accumulate(parts, float(B), st["epoch"])

    def _val_graph_batch(self, img, mask, lu, distmap, alpha, curves=False, objects=None):
        """``_val_batch`` through ``GraphReplay``: a captured graph per key, after two eager batches of that key (a
        validation set whose last batch is smaller keeps one graph per batch size).  alpha is baked into the captured
        blend: it belongs to the key where it is read (BOUNDARY-RAMPED)"""
        key = (tuple(img.shape), img.dtype, tuple(mask.shape), mask.dtype,
               None if lu is None else (tuple(lu.shape), lu.dtype),
               None if distmap is None else (tuple(distmap.shape), distmap.dtype),
               self.model.precision, self.losses, float(alpha) if "BOUNDARY-RAMPED" in self.losses else None) + \
            ((True,) if curves else ())
        self._val_buffers()              # (a moved model drops the graphs)
        if objects is not None:          # the sweep is baked into the captured launches: it belongs to the key
            key += (("objects",) + objects._key(),)
            self._obj_buffers()
        self._val_replays.get(key, lambda: GraphReplay(
            self.model.engine, lambda *batch: self._val_batch(*batch, alpha, curves, objects), warmup=2))(img, mask, lu, distmap)

    @torch.no_grad()
    def validate(self, loader, to_device=None, stage: str = "val", alpha: float = 1.0, curves: bool = False,
                 objects=None) -> dict:
        """One validation epoch: eval-mode BatchNorm in this trainer's precision; per batch the loss terms of
        ``self.losses`` and both F-scores as ``SemSegment.validation_step`` logs them, the confusion counts over all pixels
        and over ``lu == 1``.  Batches are ``(img, mask[, distmap[, lu[, stats]]])`` tuples or the datamodule's dicts;
        boundary terms get device distance maps when the loader supplies none.

        Every epoch value is the mean of the per-batch values weighted by batch size (Lightning's
        ``self.log(on_step=False, on_epoch=True)``): "{stage}/dice" is the weighted mean of per-batch F-scores, not the
        F-score of pooled counts.  Returns Python floats under "{stage}/total_loss", "/dice_loss", "/dice",
        "/dice_with_bg", "/focal_loss" and "/boundary_loss" (when those terms are on), "/batches", "/samples", and the
        four matrices of ``SemSegment.confusion_matrices`` ("cm_px", "cm_norm", "cm_px_masked", "cm_norm_masked").

        Everything accumulates on the device; the host reads one buffer when the epoch is over (with world > 1 after one
        all-reduce, so every rank sees the same numbers).  graph=True replays a captured batch (one host synchronisation
        per new key, when it is captured).  A label outside [0, K) raises the AssertionError of ``_check_labels``.
        Left as found: the train / eval flags of the model and of ``model.encoder``, the freeze, ``bn_state``,
        ``num_batches_tracked``, the parameters and the captured training graph.

        ``curves=True`` also collects, per class, the histogram of the predicted probability split by ground truth (over
        all pixels and over ``lu == 1``) and returns it under "curves" as a ``ProbabilityCurves`` (``loss/curves.py``:
        precision / recall, ROC, F1 and the best threshold of every operating point, not the arg-max alone), with the
        model's class names when it has them.  Every batch then takes the unfused chain (logits -> ``loss_forward`` ->
        ``confusion_matrix`` -> one ``prob_histogram`` of the logits): the fused ``dt_head_eval`` path is not used with
        curves because it never materialises the logits.  The counts are exact; the real-valued metrics are those of
        ``curves=False`` to fp32 summation order.  The histogram travels in the epoch's one transfer (and all-reduce) as
        fp64, exact below 2^53 like the confusion counts.  With ``curves=False`` not one launch differs from before.

        ``objects`` (an ``ObjectSweep``, ``loss/objects.py``) also collects the crown-level histogram of the hysteresis
        patches at the sweep's low thresholds against the target's crowns and returns it under "objects" as an
        ``ObjectCurves``: crown-level precision / recall / F1 for every ``(T, M)`` of a ``Decision`` at once, and
        ``best_decision()``.  Every batch takes the unfused chain as with ``curves``, then ``ops.object_histogram`` on
        ``prob_histogram``'s ``q``; with graph=True the batch is captured like every other one (the sweep is part of the
        key).  The counts travel in the same transfer and all-reduce.  Without ``objects`` not one launch, key or returned
        entry differs."""
        from .network.segmodel import create_combined_batch
        if not isinstance(curves, (bool,)):
            raise ValueError(f"validate: curves must be True or False, got {curves!r}")
        m = self.model
        K = m.spec.classes
        if objects is not None:
            from .loss.objects import check_sweep
            objects = check_sweep(objects, K, "validate")
        st = self._val_buffers()
        for t in st.values():
            t.zero_()
        if objects is not None:
            for t in self._obj_buffers().values():
                t.zero_()
        run = self._val_graph_batch if self.use_graph else self._val_batch
        batches = 0
        for batch in loader:
            batch = create_combined_batch(batch) if isinstance(batch, dict) else tuple(batch)
            if len(batch) < 2:
                raise ValueError("validate: a batch is (img, mask[, distmap[, lu[, stats]]])")
            img, mask = batch[0], batch[1]
            distmap = batch[2] if len(batch) > 2 else None
            lu = batch[3] if len(batch) > 3 else None
            if to_device:
                img, mask = img.to(to_device), mask.to(to_device)
                distmap = distmap.to(to_device) if distmap is not None else None
                lu = lu.to(to_device) if lu is not None else None
            m._require_gpu(img)
            if mask.dtype != torch.int64:
                mask = mask.long()
            if lu is not None and lu.dtype != torch.int64:
                lu = lu.long()
            if objects is not None:
                run(img, mask, lu, distmap, alpha, curves, objects)
            else:
                run(img, mask, lu, distmap, alpha, curves) if curves else run(img, mask, lu, distmap, alpha)
            batches += 1
        if batches == 0:
            raise ValueError("validate: no batches")
        # the one transfer of the epoch: nine doubles, the counts (exact in fp64 below 2^53) and the label flag
        parts = [st["epoch"], st["counts"].reshape(-1).double()]
        if curves:
            parts.append(st["hist"].reshape(-1).double())
        if objects is not None:
            parts += [self._obj_state["hist"].reshape(-1).double(), self._obj_state["targets"].double()]
        buf = torch.cat(parts + [st["err"].double()])
        if self.reducer and self.world > 1:
            self.reducer.dist.all_reduce(buf, op=self.reducer.dist.ReduceOp.SUM, group=self.reducer.group)
        host = buf.cpu()
        if float(host[-1]) != 0.0:
            raise AssertionError(f"labels outside [0, {K}) were seen this epoch (class2one_hot)")
        out = epoch_metrics(host[:9], host[9:9 + 2 * K * K].reshape(2, K, K), self.losses, stage, batches)
        if curves:
            from .loss.curves import ProbabilityCurves
            names = getattr(m, "classes", None)
            names = list(names) if isinstance(names, (list, tuple)) and len(names) == K else None
            hist = host[9 + 2 * K * K:9 + 2 * K * K + 2 * K * 2 * 256].reshape(2, K, 2, 256).to(torch.int64).numpy()
            out["curves"] = ProbabilityCurves(hist, names)
        if objects is not None:
            from .loss.objects import ObjectCurves
            names = getattr(m, "classes", None)
            names = list(names) if isinstance(names, (list, tuple)) and len(names) == K else None
            tail = host[-1 - K - K * 2 * 256 * 256:-1].to(torch.int64).numpy()
            out["objects"] = ObjectCurves(tail[:-K].reshape(K, 2, 256, 256), tail[-K:], objects, names)
        return out

    # ------------------------------------------------------------------ full state: what an exact continuation needs
    _DESCRIPTION = ("decoder", "in_channels", "classes", "n_params", "layout", "precision", "losses", "average",
                    "average_decay", "world")

    def describe(self) -> dict:
        """what must agree between the trainer that saved a state and the one that loads it (JSON-serialisable);
        "layout" is a fingerprint of the spec's (key, offset, length) list.  ``graph`` is not part of it."""
        spec, avg = self.model.spec, self.averager
        layout = hashlib.sha256(repr([(c.key, int(c.w_off), int(c.w_size)) for c in spec.convs]).encode()).hexdigest()
        return {"decoder": spec.decoder_kind, "in_channels": int(spec.in_channels), "classes": int(spec.classes),
                "n_params": int(spec.n_params), "layout": layout, "precision": self.model.precision,
                "losses": list(self.losses), "average": None if avg is None else avg.mode,
                "average_decay": None if avg is None else float(avg.decay), "world": int(self.world)}

    @torch.no_grad()
    def state_dict(self) -> dict:
        """Everything the next ``step`` depends on, downloaded: the RAW flat buffers (``flat_params`` with its alignment
        padding and the outer taps of a 1x1 head held as a 3x3 kernel, which no smp key names; ``bn_state``;
        ``num_batches_tracked``), the optimiser's and the averager's state, the module flags and ``describe()``."""
        m = self.model
        return {"description": self.describe(),
                "flat_params": m.flat_params.detach().cpu(), "bn_state": m.bn_state.detach().cpu(),
                "num_batches_tracked": m.num_batches_tracked.detach().cpu(),
                "opt": self.opt.state_dict(),
                "averager": None if self.averager is None else self._need_averager("state_dict").state_dict(),
                "flags": {"encoder_frozen": bool(m.encoder_frozen), "encoder_training": bool(m.encoder.training),
                          "training": bool(m.training)}}

    def check_state_dict(self, sd: dict):
        """ValueError naming the first field of the description that differs (RuntimeError for a tensor of another
        length); reads only"""
        mine, theirs = self.describe(), sd.get("description")
        if not isinstance(theirs, dict):
            raise ValueError("load_state_dict: not a HipTrainer state (no description)")
        for field in self._DESCRIPTION:
            if theirs.get(field) != mine[field]:
                raise ValueError(f"load_state_dict: {field} differs: the state was saved with {theirs.get(field)!r}, this "
                                 f"trainer has {mine[field]!r}")
        m = self.model
        for name, t in (("flat_params", m.flat_params), ("bn_state", m.bn_state),
                        ("num_batches_tracked", m.num_batches_tracked)):
            if sd[name].numel() != t.numel():
                raise RuntimeError(f"load_state_dict: {name} of {sd[name].numel()} elements, the model's has {t.numel()}")
        self.opt.check_state_dict(sd["opt"])
        if self.averager is not None and sd["averager"]["avg"].numel() != self.averager.avg.numel():
            raise RuntimeError(f"load_state_dict: average of {sd['averager']['avg'].numel()} floats, "
                               f"this trainer's has {self.averager.avg.numel()}")

    @torch.no_grad()
    def load_state_dict(self, sd: dict):
        """Continue where ``state_dict()`` was taken, on this trainer's own tensors.  The description is checked first
        (ValueError, nothing modified).  Every tensor is then written IN PLACE — the optimiser, the averager and the
        engine hold views of these buffers — the engine's weight images are marked stale, and the step, recalibration and
        validation replay caches are dropped: their graphs were captured on another trajectory's partition and flags, so
        the next ``step`` warms up and captures again on the restored state (``static_batch()`` is None until then)."""
        self.check_state_dict(sd)
        m = self.model
        dev = m.flat_params.device
        m.flat_params.data.copy_(sd["flat_params"].to(dev, torch.float32).view(-1))
        m.bn_state.copy_(sd["bn_state"].to(dev, torch.float32).view(-1))
        m.num_batches_tracked.copy_(sd["num_batches_tracked"].to(dev, torch.int64).view(-1))
        self.opt.load_state_dict(sd["opt"])
        if self.averager is not None:
            self._need_averager("load_state_dict").load_state_dict(sd["averager"])
        flags = sd["flags"]
        m.train(bool(flags["training"]))                     # (recurses into the encoder view: its own flag comes after)
        m.encoder.train(bool(flags["encoder_training"]))
        m.encoder_frozen = bool(flags["encoder_frozen"])
        m.engine.mark_weights_changed()
        self._step_replays.clear()
        self._recal_replays.clear()
        self._val_replays.clear()
        self.last = {}

    def step(self, img: torch.Tensor, mask: torch.Tensor, distmap: Optional[torch.Tensor] = None,
             alpha: float = 1.0):
        """returns the (device) loss tensor; no host synchronisation happens here.  Honours ``model.encoder``: its
        BatchNorm mode (``model.encoder.eval()`` survives the step) and its weight freeze (frozen ranges get no
        gradient, no all-reduce and no update)."""
        self.opt.set_trainable(self.model.trainable_ranges())
        if self.use_graph:
            return self._graph_step(img, mask, distmap, alpha)
        return self._eager_step(img, mask, distmap, alpha)

    # ------------------------------------------------------------------ HIP-graph replay of the whole step
    def _graph_step(self, img, mask, distmap, alpha):
        # alpha (the per-epoch boundary ramp of segmodel.py:157-160) is baked into the captured loss blend: it belongs to
        # the key only where it is read (BOUNDARY-RAMPED) — otherwise fit()'s ramp would re-capture the step every epoch
        # the encoder's freeze and BatchNorm mode change what the step launches: a change re-captures
        key = (tuple(img.shape), img.dtype, tuple(mask.shape), mask.dtype,
               None if distmap is None else tuple(distmap.shape),
               float(alpha) if "BOUNDARY-RAMPED" in self.losses else None,
               self.model.encoder_frozen, self.model.encoder.training or not self.model.training)

        def step_last(img, mask, distmap, capturing=False):      # -> ``self.last`` of that step: what a replay hands back
            self._eager_step(img, mask, distmap, alpha, capturing=capturing)
            return self.last
        r = self._step_replays.get(key, lambda: GraphReplay(self.model.engine, step_last, warmup=2,
                                                            capture_fn=partial(step_last, capturing=True)))
        # two eager warm-up steps (real steps, with their own bookkeeping), then GraphReplay captures on its static
        # buffers.  A loader that writes its batches straight into them (`static_batch()`) hands them back here: nothing
        # to copy (at B = 64 the image copy alone is 201 MB = 0.2 ms of a 25 ms step)
        self.opt.sync_lr()                   # never inside a capture: a changed learning rate reaches the replay via lr_dev
        t_host = self.opt.t
        last = r(img, mask, distmap)
        if r.captured:
            self.opt.t = t_host + 1          # host mirror (a capture launches nothing); the device's t_dev is authoritative
            self.model.engine.mark_weights_changed()
            self.model._bn_tracked_inc()     # module bookkeeping outside the graph (smp state_dict key)
            self.last = last
        return last["loss"]

    def static_batch(self):
        """(img, mask, distmap) buffers the captured step reads — available once the graph exists (after the eager
        warm-up steps); a data pipeline that fills THESE tensors (H2D copies, device-side augmentation) and passes them
        to ``step`` saves the per-step staging copy.  None before capture or without graph replay."""
        r = next(iter(self._step_replays.values()), None)
        if not self.use_graph or r is None or not r.captured:
            return None
        return r.inputs

    def _eager_step(self, img, mask, distmap, alpha, capturing: bool = False):
        """forward -> fused loss -> hand-scheduled backward -> (all-reduce) -> clip + Adam, straight on the C ABI:
        no autograd graph, no ATen arithmetic; every launch is the same for every step (HIP-graph capturable)."""
        m, eng, opt = self.model, self.model.engine, self.opt
        if not m.training:       # (a model put in eval() as a whole trains as before; model.encoder.eval() survives)
            m.train()
        m._require_gpu(img)
        enc_tr, frozen = m._encoder_training(), m.encoder_frozen
        params = m.flat_params.detach()
        grads = m._grad_buffer()
        with torch.no_grad():
            x = img if img.dtype == torch.float32 else img.float()
            if m.precision == "bf16":
                logits = eng.forward_bf16_train(x, params, m.bn_state, enc_training=enc_tr, enc_frozen=frozen)
            else:
                logits, _ = eng.forward(x, params, m.bn_state, True, save=True, enc_training=enc_tr, enc_frozen=frozen)
            if not capturing:
                m._bn_tracked_inc()
            if distmap is None and any(n.startswith("BOUNDARY") for n in self.losses):
                distmap = distmaps_on_device(mask, logits.shape[1])
            parts, err, saved = loss_forward(logits, mask, distmap, {"losses": self.losses, "alpha": alpha})
            dl = loss_backward(saved)
            if m.precision == "bf16":
                eng.backward_bf16(dl, params, grads)
            else:
                eng.backward(dl, params, grads)
            if self.reducer:
                self.reducer.wait()
            # non-finite loss -> skip the update (reference segmodel.py:220-222 returns None).  The decision must be
            # GLOBAL: the gradient buckets are already summed over the replicas, so one rank's NaN poisons everyone's
            # update — all ranks skip together (one 4-byte MAX all-reduce on the same group)
            loss = parts[7]
            skip = opt.skip_from_loss(loss)
            if self.reducer and self.world > 1:
                self.reducer.dist.all_reduce(skip, op=self.reducer.dist.ReduceOp.MAX, group=self.reducer.group)
            norm = opt.step(grads, grad_scale=1.0 / self.world, skip_flag=skip, capturing=capturing)
            if self.averager is not None and self.averager.mode == "ema":
                self._need_averager("step").update(skip_flag=skip, capturing=capturing)
        eng.mark_weights_changed()   # the fused optimiser wrote the flat buffer behind torch's version counter
        self.last = {"loss": loss, "parts": {k: parts[i] for i, k in enumerate(PART_KEYS)}, "grad_norm": norm,
                     "label_error": err, "skipped": skip}
        return loss


class _TrainerView:
    """what a Lightning callback's ``on_train_epoch_start(trainer, pl_module)`` reads from ``trainer``:
    ``current_epoch``, ``optimizers`` (assigning a new ``torch.optim.Adam`` resets the fused optimiser's state and takes
    its lr as the new base lr) and ``lr_schedulers`` (assigning a ``CosineAnnealingLR`` restarts the cosine schedule from
    the current epoch with its T_max)."""

    def __init__(self, trainer: "HipTrainer", sched: dict):
        self._trainer, self._sched = trainer, sched
        self.current_epoch = 0
        self.optimizer_frequencies = []

    @property
    def optimizers(self):
        return [self._trainer.opt]

    @optimizers.setter
    def optimizers(self, opts):
        opt = opts[0] if isinstance(opts, (list, tuple)) else opts
        lr = float(opt.param_groups[0]["lr"]) if hasattr(opt, "param_groups") else float(opt.lr)
        self._trainer.opt.reset_state(lr=lr)
        self._sched.update(base_lr=lr, start=self.current_epoch)

    @property
    def lr_schedulers(self):
        return [self._sched]

    @lr_schedulers.setter
    def lr_schedulers(self, scheds):
        s = scheds[0] if isinstance(scheds, (list, tuple)) else scheds
        s = s.get("scheduler", s) if isinstance(s, dict) else s
        if hasattr(s, "T_max"):
            self._sched.update(t_max=int(s.T_max), start=self.current_epoch)

    def _configure_schedulers(self, schedulers, monitor=None, is_manual_optimization=False):
        return list(schedulers)     # (Lightning's own wrapping is not needed here)


class _ModuleView:
    """what such a callback reads from ``pl_module``: ``model`` (with ``model.encoder``), ``encoder_weights``,
    ``hparams.training.*`` and ``parameters()``"""

    def __init__(self, model, encoder_weights, hparams):
        self.model = model
        self.encoder_weights = encoder_weights
        self.hparams = hparams

    def parameters(self):
        return self.model.parameters()


@dataclass
class SWAConfig:
    """stochastic weight averaging in ``fit``: averaging and the ``SWALR`` schedule start at epoch ``swa_start``;
    ``swa_lr`` None = the base learning rate"""
    swa_start: int
    swa_lr: Optional[float] = None
    anneal_epochs: int = 10
    anneal_strategy: str = "cos"


def swa_lr(epoch_in_swa: int, lr_at_start: float, swa_lr: float, anneal_epochs: int = 10, strategy: str = "cos") -> float:
    """closed form of ``torch.optim.swa_utils.SWALR`` stepped once per epoch: ``epoch_in_swa`` = 0 in the first SWA
    epoch (the rate the schedule before it had reached), ``swa_lr`` from ``anneal_epochs`` on"""
    if strategy not in ("cos", "linear"):
        raise ValueError(f"anneal_strategy {strategy!r}: use 'cos' or 'linear'")
    if epoch_in_swa < 0 or anneal_epochs < 0:
        raise ValueError("swa_lr: epoch_in_swa and anneal_epochs must not be negative")
    t = 1.0 if anneal_epochs == 0 else min(1.0, epoch_in_swa / anneal_epochs)
    a = (1.0 - math.cos(math.pi * t)) / 2.0 if strategy == "cos" else t
    return swa_lr * a + lr_at_start * (1.0 - a)


def resolve_swa(swa, epochs: int, base_lr: float) -> Optional[SWAConfig]:
    """``fit``'s swa argument -> a checked SWAConfig (None stays None).  True = the defaults Lightning documents for
    ``stochastic_weight_avg: True``: start at int(0.8 * epochs), 10 annealing epochs, cosine, swa_lr = the base rate."""
    if swa is None or swa is False:
        return None
    cfg = SWAConfig(swa_start=int(0.8 * epochs)) if swa is True else swa
    if not isinstance(cfg, SWAConfig):
        raise ValueError(f"fit(swa=...): None, True or an SWAConfig, not {type(swa).__name__}")
    lr = float(base_lr) if cfg.swa_lr is None else float(cfg.swa_lr)
    if int(cfg.swa_start) != cfg.swa_start or cfg.swa_start < 0:
        raise ValueError(f"swa_start {cfg.swa_start!r}: an epoch number >= 0")
    if cfg.swa_start >= epochs:
        raise ValueError(f"swa_start {cfg.swa_start} >= epochs {epochs}: nothing would be averaged")
    if int(cfg.anneal_epochs) != cfg.anneal_epochs or cfg.anneal_epochs < 0:
        raise ValueError(f"anneal_epochs {cfg.anneal_epochs!r}: an integer >= 0")
    if not lr >= 0.0:
        raise ValueError(f"swa_lr {cfg.swa_lr!r} must not be negative")
    if cfg.anneal_strategy not in ("cos", "linear"):
        raise ValueError(f"anneal_strategy {cfg.anneal_strategy!r}: use 'cos' or 'linear'")
    return SWAConfig(int(cfg.swa_start), lr, int(cfg.anneal_epochs), cfg.anneal_strategy)


_EPOCH_SLOTS = {"dice_loss": 0, "boundary_loss": 1, "focal_loss": 2, "dice": 4, "dice_with_bg": 5, "total_loss": 6}


def validation_keys(losses: Sequence[str], stage: str = "val") -> tuple:
    """the scalar keys ``HipTrainer.validate`` returns for a loss list (what a monitor may name)"""
    names = ["total_loss", "dice_loss", "dice", "dice_with_bg"]
    if "FOCAL" in losses:
        names.append("focal_loss")
    if any(n.startswith("BOUNDARY") for n in losses):
        names.append("boundary_loss")
    return tuple(f"{stage}/{n}" for n in names + ["batches", "samples"])


def epoch_metrics(epoch, counts, losses: Sequence[str], stage: str, batches: int) -> dict:
    """host side of a validation epoch.  epoch: nine doubles — sum_b w_b * parts_b[i] for the eight ``parts`` of the
    loss algebra and sum_b w_b (w_b = batch size); the epoch value of a key is their quotient, Lightning's mean of
    ``self.log(on_step=False, on_epoch=True)`` values weighted by batch size.  counts [2,K,K] -> the four matrices of
    ``SemSegment.confusion_matrices``."""
    epoch = [float(v) for v in epoch]
    wsum = epoch[8]
    if not wsum > 0.0:
        raise ValueError("epoch_metrics: the weights sum to zero")
    out = {}
    for key in validation_keys(losses, stage):
        name = key[len(stage) + 1:]
        if name in _EPOCH_SLOTS:
            out[key] = epoch[_EPOCH_SLOTS[name]] / wsum
    out[f"{stage}/batches"] = float(batches)
    out[f"{stage}/samples"] = wsum
    cm = torch.as_tensor(counts).double()
    for name, mat in (("", cm[0]), ("_masked", cm[1])):
        out[f"cm_px{name}"] = mat.to(torch.int64)
        out[f"cm_norm{name}"] = mat / mat.sum(dim=1, keepdim=True).clamp_min(1.0)
    return out


@dataclass
class CheckpointConfig:
    """``ModelCheckpoint`` of the reference's configs/callbacks/default.yaml: keep the ``save_top_k`` best files by
    ``monitor`` under ``dirpath`` (``filename`` is formatted with ``epoch``; ".ckpt" is appended) and ``last.ckpt``"""
    dirpath: str
    monitor: str = "val/dice"
    mode: str = "max"
    save_top_k: int = 1
    save_last: bool = True
    filename: str = "epoch_{epoch:03d}"


@dataclass
class EarlyStoppingConfig:
    """``EarlyStopping`` of the reference's configs/callbacks/default.yaml"""
    monitor: str = "val/dice"
    mode: str = "max"
    patience: int = 200
    min_delta: float = 0.0


def _check_monitor(what: str, monitor, mode, losses, stage: str = "val", extra: Sequence[str] = ()):
    if mode not in ("min", "max"):
        raise ValueError(f"{what}: mode {mode!r}: use 'min' or 'max'")
    keys = [k for k in validation_keys(losses, stage) if not k.endswith(("/batches", "/samples"))] + list(extra)
    if monitor not in keys:
        raise ValueError(f"{what}: monitor {monitor!r} is not a validation metric of losses {tuple(losses)}: {keys}")


def resolve_checkpoint(cfg, losses: Sequence[str], extra: Sequence[str] = ()) -> Optional[CheckpointConfig]:
    """``fit``'s checkpoint argument -> a checked CheckpointConfig (None stays None); ``extra``: further scalars the monitor may
    name (the crown-level ones of ``fit(objects=...)``)"""
    if cfg is None:
        return None
    if not isinstance(cfg, CheckpointConfig):
        raise ValueError(f"fit(checkpoint=...): None or a CheckpointConfig, not {type(cfg).__name__}")
    _check_monitor("checkpoint", cfg.monitor, cfg.mode, losses, extra=extra)
    if isinstance(cfg.save_top_k, bool) or int(cfg.save_top_k) != cfg.save_top_k or cfg.save_top_k < 0:
        raise ValueError(f"save_top_k {cfg.save_top_k!r}: an integer >= 0")
    if not cfg.dirpath:
        raise ValueError("checkpoint: dirpath is required")
    try:
        name = cfg.filename.format(epoch=0)
    except (KeyError, IndexError, ValueError) as e:
        raise ValueError(f"checkpoint: filename {cfg.filename!r} must format with epoch alone") from e
    if not name or os.sep in name or name == "last":
        raise ValueError(f"checkpoint: filename {cfg.filename!r}: a plain file name other than 'last'")
    return CheckpointConfig(str(cfg.dirpath), cfg.monitor, cfg.mode, int(cfg.save_top_k), bool(cfg.save_last), cfg.filename)


def resolve_early_stopping(cfg, losses: Sequence[str], extra: Sequence[str] = ()) -> Optional[EarlyStoppingConfig]:
    """``fit``'s early_stopping argument -> a checked EarlyStoppingConfig (None stays None); ``extra`` as in
    ``resolve_checkpoint``"""
    if cfg is None:
        return None
    if not isinstance(cfg, EarlyStoppingConfig):
        raise ValueError(f"fit(early_stopping=...): None or an EarlyStoppingConfig, not {type(cfg).__name__}")
    _check_monitor("early_stopping", cfg.monitor, cfg.mode, losses, extra=extra)
    if isinstance(cfg.patience, bool) or int(cfg.patience) != cfg.patience or cfg.patience < 0:
        raise ValueError(f"patience {cfg.patience!r}: an integer >= 0")
    if not float(cfg.min_delta) >= 0.0:
        raise ValueError(f"min_delta {cfg.min_delta!r} must not be negative")
    return EarlyStoppingConfig(cfg.monitor, cfg.mode, int(cfg.patience), float(cfg.min_delta))


class ModelSelection:
    """Best-checkpoint bookkeeping and early stopping over the validated epochs of ``fit`` — the rules of Lightning's
    ``ModelCheckpoint`` / ``EarlyStopping``, restated from their documentation (unpinned: Lightning is not installed):

    top-k: a score enters only if fewer than k are kept or it is STRICTLY better than the worst kept one (a tie keeps
    the earlier file); the dropped file is deleted; a non-finite score is never kept.  ``last.ckpt`` is rewritten after
    every validated epoch.  Early stopping: an improvement is ``score - min_delta > best`` (mode max; mirrored for min);
    otherwise a counter goes up and training stops after the epoch in which it reaches ``patience``; a non-finite
    monitored value stops at once.

    save(path) writes one checkpoint file; write=False (ranks other than 0) takes the same decisions without files."""

    def __init__(self, checkpoint: Optional[CheckpointConfig], early_stopping: Optional[EarlyStoppingConfig],
                 save: Callable[[str], None], write: bool = True):
        self.ck, self.es, self.save, self.write = checkpoint, early_stopping, save, write
        self.kept: List = []             # [(score, path)] of the top-k files
        self.best_model_path: Optional[str] = None
        self.best_model_score: Optional[float] = None
        self.last_model_path: Optional[str] = None
        self.es_best = None if early_stopping is None else (-math.inf if early_stopping.mode == "max" else math.inf)
        self.wait = 0
        self.stopped_epoch: Optional[int] = None
        if checkpoint is not None and write:
            os.makedirs(checkpoint.dirpath, exist_ok=True)

    @staticmethod
    def _better(a: float, b: float, mode: str) -> bool:
        return a > b if mode == "max" else a < b

    def _monitored(self, cfg, metrics: dict) -> float:
        if cfg.monitor not in metrics:
            raise KeyError(f"monitor {cfg.monitor!r} is not among the validation metrics {sorted(metrics)}")
        return float(metrics[cfg.monitor])

    def update(self, epoch: int, metrics: dict) -> bool:
        """after a validated epoch: write / delete files, count patience -> True when training should stop"""
        ck, es = self.ck, self.es
        if ck is not None:
            score = self._monitored(ck, metrics)
            if ck.save_top_k > 0 and math.isfinite(score):
                worst = None
                for e in self.kept:      # the worst kept score; among equals the latest file goes first
                    if worst is None or not self._better(e[0], worst[0], ck.mode):
                        worst = e
                if len(self.kept) < ck.save_top_k or self._better(score, worst[0], ck.mode):
                    path = os.path.join(ck.dirpath, ck.filename.format(epoch=epoch) + ".ckpt")
                    if self.write:
                        self.save(path)
                    self.kept.append((score, path))
                    if len(self.kept) > ck.save_top_k:
                        self.kept.remove(worst)
                        if self.write and os.path.exists(worst[1]):
                            os.remove(worst[1])
                    best = self.kept[0]
                    for e in self.kept[1:]:
                        if self._better(e[0], best[0], ck.mode):
                            best = e
                    self.best_model_score, self.best_model_path = best
            if ck.save_last:
                self.last_model_path = os.path.join(ck.dirpath, "last.ckpt")
                if self.write:
                    self.save(self.last_model_path)
        if es is None:
            return False
        score = self._monitored(es, metrics)
        if not math.isfinite(score):
            self.stopped_epoch = epoch
            return True
        improved = score - es.min_delta > self.es_best if es.mode == "max" else score + es.min_delta < self.es_best
        if improved:
            self.es_best, self.wait = score, 0
        else:
            self.wait += 1
            if self.wait >= es.patience:
                self.stopped_epoch = epoch
                return True
        return False

    def state_dict(self) -> dict:
        """the decisions so far, JSON-serialisable (``es_best`` starts at +-inf: Python's ``json`` round-trips ``Infinity``
        and ``NaN``).  The configuration is not part of it: a resumed run brings its own."""
        return {"kept": [[float(s), str(p)] for s, p in self.kept],
                "best_model_path": self.best_model_path, "best_model_score": self.best_model_score,
                "last_model_path": self.last_model_path, "es_best": self.es_best, "wait": int(self.wait),
                "stopped_epoch": self.stopped_epoch}

    def load_state_dict(self, sd: dict):
        self.kept = [(float(s), str(p)) for s, p in sd["kept"]]
        self.best_model_path, self.last_model_path = sd["best_model_path"], sd["last_model_path"]
        self.best_model_score = None if sd["best_model_score"] is None else float(sd["best_model_score"])
        self.es_best = None if sd["es_best"] is None else float(sd["es_best"])
        self.wait = int(sd["wait"])
        self.stopped_epoch = None if sd["stopped_epoch"] is None else int(sd["stopped_epoch"])


def _generic_hparams(trainer, training_conf: Optional[dict] = None) -> dict:
    """hyper-parameters of a checkpoint from the model's own configuration (``checkpoint_writer`` without a module)"""
    from .utils.config import default_network, default_training
    model = trainer if isinstance(trainer, UNetHIP) else trainer.model
    K = model.spec.classes
    classes = ["background", "deadtree"] if K == 2 else ["background"] + [f"class{i}" for i in range(1, K)]
    net = dict(default_network(architecture=model.spec.decoder_kind, in_channels=model.spec.in_channels, classes=classes,
                               losses=list(getattr(trainer, "losses", ("GDICE", "FOCAL")))))
    if model.spec.decoder_kind == "efficientunetplusplus":
        net.update(squeeze_ratio=model.spec.squeeze_ratio, expansion_ratio=model.spec.expansion_ratio)
    return {"network": net, "training": dict(default_training(**(training_conf or {})))}


def checkpoint_payload(trainer: "HipTrainer", pl_module=None, training_conf: Optional[dict] = None) -> dict:
    """what ``checkpoint_writer``'s file holds, as a dict: ``state_dict`` (smp names, ``model.`` prefix) and
    ``hyper_parameters_json`` — the module's own when ``pl_module`` has ``save_checkpoint`` and ``hparams``"""
    if pl_module is not None and hasattr(pl_module, "save_checkpoint") and hasattr(pl_module, "hparams"):
        model = pl_module.model
        hp = {"network": dict(pl_module.hparams["network"]), "training": dict(pl_module.hparams["training"])}
    else:
        model = trainer if isinstance(trainer, UNetHIP) else trainer.model
        hp = _generic_hparams(trainer, training_conf)
    sd = {f"model.{k}": v for k, v in model.smp_state_dict().items()}
    return {"state_dict": sd, "hyper_parameters_json": json.dumps(hp)}


def checkpoint_writer(trainer: "HipTrainer", pl_module=None, training_conf: Optional[dict] = None) -> Callable[[str], None]:
    """path -> one ``.ckpt`` in ``SemSegment.save_checkpoint``'s payload (``SemSegment.load_from_checkpoint`` and
    ``PyTorchInference(path)`` read it).  With a ``pl_module`` that has ``save_checkpoint``: that method.  Otherwise
    the same payload from the model's own configuration: architecture, channels and class count of its spec, the
    trainer's loss list, ``encoder_weights`` None (the file holds the encoder's tensors; nothing is to be fetched again).
    `trainer` may be the ``UNetHIP`` itself: an inference-only model (EfficientUnet++ decoder, say one converted from a
    reference checkpoint) has no trainer; its file records the default loss list and the decoder's two ratios."""
    if pl_module is not None and hasattr(pl_module, "save_checkpoint"):
        return pl_module.save_checkpoint
    model = trainer if isinstance(trainer, UNetHIP) else trainer.model
    hp = _generic_hparams(trainer, training_conf)

    def save(path):
        sd = {f"model.{k}": v for k, v in model.smp_state_dict().items()}
        torch.save({"state_dict": sd, "hyper_parameters_json": json.dumps(hp)}, str(path))
    return save


@dataclass
class StateConfig:
    """``fit(state=...)``: the full training state goes to ``path`` after every ``every_n_epochs``-th epoch"""
    path: str
    every_n_epochs: int = 1


def resolve_state(cfg) -> Optional[StateConfig]:
    """``fit``'s state argument (None, a path or a StateConfig) -> a checked StateConfig (None stays None)"""
    if cfg is None:
        return None
    if isinstance(cfg, (str, os.PathLike)):
        cfg = StateConfig(os.fspath(cfg))
    if not isinstance(cfg, StateConfig):
        raise ValueError(f"fit(state=...): None, a path or a StateConfig, not {type(cfg).__name__}")
    if not isinstance(cfg.path, (str, os.PathLike)) or not os.fspath(cfg.path):
        raise ValueError(f"state: path {cfg.path!r}: a file path")
    n = cfg.every_n_epochs
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"state: every_n_epochs {n!r}: an integer >= 1")
    return StateConfig(os.fspath(cfg.path), n)


def _swa_record(swa: Optional[SWAConfig]):
    return None if swa is None else {"swa_start": swa.swa_start, "swa_lr": swa.swa_lr, "anneal_epochs": swa.anneal_epochs,
                                     "anneal_strategy": swa.anneal_strategy}


def _check_resume(file: dict, path, trainer, epochs: int, base_lr: float, t_max: int, swa, overrides: bool) -> dict:
    """everything ``fit(resume=...)`` refuses, checked on the loaded file before anything is modified -> the fit state"""
    fs = file["fit"]
    saved = int(fs["epoch"])
    if fs["stopped"]:
        raise ValueError(f"resume {path}: that run had stopped after epoch {saved} (early stopping): nothing is left to "
                         "continue")
    if saved + 1 >= epochs:
        raise ValueError(f"resume {path}: epoch {saved} of that run is complete and epochs is {epochs}: nothing is left "
                         "to run; pass a larger epochs")
    if _swa_record(swa) != fs["swa"]:
        raise ValueError(f"resume {path}: swa differs: the state was saved under {fs['swa']!r}, this call resolves to "
                         f"{_swa_record(swa)!r}")
    if not overrides:
        for name, mine in (("base_lr", float(base_lr)), ("t_max", int(t_max))):
            if fs[name] != mine:
                raise ValueError(f"resume {path}: {name} differs: saved {fs[name]!r}, this call {mine!r} "
                                 "(resume_overrides=True takes this call's)")
    trainer.check_state_dict(file["trainer"])
    return fs


def fit(trainer: HipTrainer, loader, epochs: int, base_lr: float = 3e-4, t_max: int = 10, to_device=None,
        on_epoch_end=None, callbacks=None, pl_module=None, swa=None, val_loader=None, check_val_every_n_epoch: int = 1,
        checkpoint=None, early_stopping=None, curves: bool = False, objects=None, state=None, resume=None,
        resume_overrides: bool = False):
    """Minimal stand-in for ``Trainer.fit`` on the hot path (reference deadtrees/train.py:113): per-batch
    ``HipTrainer.step`` and the per-epoch ``CosineAnnealingLR(T_max)`` of segmodel.py:426-428.

    callbacks: objects with ``on_train_epoch_start(trainer, pl_module)`` (e.g. ``MultiStage``), called at the start of
    every epoch with views of this trainer and of ``pl_module`` (a ``SemSegment``; default: a view of the trainer's model
    with ``encoder_weights`` taken from the model and ``hparams.training`` = learning_rate / cosineannealing_tmax).

    val_loader: after every ``check_val_every_n_epoch``-th epoch ``trainer.validate(val_loader)`` runs (with that epoch's
    boundary ramp ``alpha``) and its scalar metrics go into the epoch's history record.  Validation leaves every module
    mode as it found it, so an encoder put in eval mode stays there (Lightning >= 1.5 puts the whole module back in
    train mode after a validation run).  checkpoint: a ``CheckpointConfig`` — the best ``save_top_k`` files by its monitor
    and ``last.ckpt``, in ``SemSegment.save_checkpoint``'s format (``pl_module.save_checkpoint`` when it has one), written
    by rank 0; the history then ends with a {"checkpoint/best_model_path", "checkpoint/best_model_score"} record.
    early_stopping: an ``EarlyStoppingConfig`` — the loop ends after the epoch in which patience runs out (or the
    monitored value is not finite).  The rules are those of ``ModelSelection``.  Validation sees the current weights,
    not the SWA average (as under Lightning's SWA callback); the SWA swap and recalibration run after the loop.
    curves=True: ``validate(..., curves=True)``; the ``ProbabilityCurves`` object stays out of the history (as the ``cm_*``
    matrices do) and its scalars go in, for every class c >= 1: "val/ap_<c>", "val/roc_auc_<c>", "val/best_f1_<c>" and
    "val/best_threshold_<c>" (the float T / 65535).  Monitors stay restricted to ``validation_keys``.
    objects: an ``ObjectSweep`` (``loss/objects.py``) — ``validate(..., objects=...)``; the ``ObjectCurves`` object stays out of
    the history and its ``summary("val")`` scalars go in ("val/crown_ap_<c>", "val/crown_best_f1_<c>",
    "val/crown_best_threshold_<c>", "val/crown_best_min_confidence_<c>", "val/crown_targets_<c>").  With ``objects``, and
    only then, a monitor may also name "val/crown_best_f1_<c>" or "val/crown_ap_<c>": the best checkpoint by crown score
    (``nan``, a class without target crowns, is "not finite": ``ModelSelection``'s rule).

    swa: None | True | SWAConfig — the loop of torch's SWA documentation on a ``HipTrainer(average="swa")``: epochs before
    ``swa_start`` keep the cosine schedule (or whatever a callback put in its place); from ``swa_start`` the rate follows
    ``swa_lr`` (SWALR, annealing from the rate the schedule had reached) and the average is updated at the end of every
    epoch; after the last epoch the average is swapped in and the BatchNorm statistics are recomputed over ``loader``.
    The history then carries "swa/n_averaged" per epoch and a final {"swa/bn_batches": k} record.

    state: a path or a ``StateConfig`` — after every ``every_n_epochs``-th epoch the full training state
    (``utils.train_state.save_training_state``: the trainer's ``state_dict()``, the schedule, the SWA hand-over rate, the
    selection state, the history, and the weights as any checkpoint holds them) replaces the file at that path, after
    the epoch's validation and model selection and before ``on_epoch_end``; rank 0 writes.
    resume: such a file.  ``epochs`` stays the total: the trainer is restored, the schedule, history and selection state
    are taken from the file, ``loader.set_epoch`` is called where the loader has it, and the loop starts at the saved
    epoch + 1.  Callbacks see ``current_epoch`` continue; stages that have passed are not run again, their effects are in
    the restored state.  Because the training step is run-to-run bit-identical, the resumed run's parameters, optimiser
    state and history equal the uninterrupted run's.  Refused with ValueError before anything is modified: a run that
    had stopped, ``saved + 1 >= epochs``, another resolved ``swa``, another ``base_lr`` / ``t_max`` (unless
    ``resume_overrides=True``: this call's values then replace the schedule's) and a trainer of another description
    (``HipTrainer.describe``).  Without ``state`` and ``resume`` nothing differs."""
    from .network.segmodel import cosine_lr, create_combined_batch
    from .utils.config import to_attrdict
    state = resolve_state(state)
    if resume is not None and (not isinstance(resume, (str, os.PathLike)) or not os.fspath(resume)):
        raise ValueError(f"fit(resume=...): None or the path of a training state file, not {resume!r}")
    if not isinstance(resume_overrides, bool):
        raise ValueError(f"fit(resume_overrides=...): True or False, not {resume_overrides!r}")
    if resume_overrides and resume is None:
        raise ValueError("fit(resume_overrides=True) without resume")
    swa = resolve_swa(swa, epochs, base_lr)
    if swa is not None and (getattr(trainer, "averager", None) is None or trainer.averager.mode != "swa"):
        raise ValueError("fit(swa=...) needs HipTrainer(average='swa')")
    if objects is not None:
        from .loss.objects import check_sweep, crown_monitors
        objects = check_sweep(objects, trainer.model.spec.classes, "fit(objects=...)")
        if val_loader is None:
            raise ValueError("fit(objects=...) collects its histogram during validation: give val_loader")
    if checkpoint is not None or early_stopping is not None:      # (a plain loop asks nothing new of `trainer`)
        crown = {} if objects is None else {"extra": crown_monitors(trainer.model.spec.classes)}
        checkpoint = resolve_checkpoint(checkpoint, trainer.losses, **crown)
        early_stopping = resolve_early_stopping(early_stopping, trainer.losses, **crown)
    if not isinstance(curves, bool):
        raise ValueError(f"fit(curves=...): True or False, not {curves!r}")
    if curves and val_loader is None:
        raise ValueError("fit(curves=True) collects its histograms during validation: give val_loader")
    if int(check_val_every_n_epoch) != check_val_every_n_epoch or check_val_every_n_epoch < 1:
        raise ValueError(f"check_val_every_n_epoch {check_val_every_n_epoch!r}: an integer >= 1")
    if val_loader is None and (checkpoint is not None or early_stopping is not None):
        raise ValueError("fit(checkpoint=... / early_stopping=...) monitor a validation metric: give val_loader")
    resumed = None
    if resume is not None:
        from .utils.train_state import load_training_state
        file = load_training_state(resume)
        resumed = _check_resume(file, resume, trainer, epochs, base_lr, t_max, swa, resume_overrides)
    select = None
    if checkpoint is not None or early_stopping is not None:
        rank0 = trainer.world == 1 or trainer.reducer.dist.get_rank(trainer.reducer.group) == 0
        select = ModelSelection(checkpoint, early_stopping,
                                checkpoint_writer(trainer, pl_module, {"learning_rate": base_lr, "cosineannealing_tmax": t_max}),
                                write=rank0)
    swa_from = None       # the rate the schedule had reached when SWA took over
    history = []
    sched = {"base_lr": float(base_lr), "t_max": int(t_max), "start": 0}
    tview = _TrainerView(trainer, sched)
    if callbacks and pl_module is None:
        hp = to_attrdict({"training": {"learning_rate": base_lr, "cosineannealing_tmax": t_max}})
        pl_module = _ModuleView(trainer.model, getattr(trainer.model, "encoder_weights", None), hp)
    elif callbacks and not hasattr(pl_module, "model"):
        raise ValueError("fit(callbacks=...): pl_module must have .model")
    first = 0
    if resumed is not None:
        trainer.load_state_dict(file["trainer"])
        del file
        first = int(resumed["epoch"]) + 1
        history = [dict(rec) for rec in resumed["history"]]
        swa_from = resumed["swa_from"]
        sched.update(base_lr=float(resumed["sched"]["base_lr"]), t_max=int(resumed["sched"]["t_max"]),
                     start=int(resumed["sched"]["start"]))
        if resume_overrides:              # this call's values replace the schedule's where they differ from the saved call's
            if float(base_lr) != resumed["base_lr"]:
                sched["base_lr"] = float(base_lr)
            if int(t_max) != resumed["t_max"]:
                sched["t_max"] = int(t_max)
        if select is not None and resumed["selection"] is not None:
            select.load_state_dict(resumed["selection"])
        if hasattr(loader, "set_epoch"):
            loader.set_epoch(int(resumed["loader_next_epoch"]))
    for epoch in range(first, epochs):
        tview.current_epoch = epoch
        for cb in callbacks or ():
            if hasattr(cb, "on_train_epoch_start"):
                cb.on_train_epoch_start(tview, pl_module)
        lr = cosine_lr(sched["base_lr"], epoch - sched["start"], sched["t_max"])
        if swa is not None and epoch >= swa.swa_start:
            swa_from = lr if swa_from is None else swa_from
            lr = swa_lr(epoch - swa.swa_start, swa_from, swa.swa_lr, swa.anneal_epochs, swa.anneal_strategy)
        trainer.opt.lr = lr
        losses = []
        alpha = min((epoch + 1) * 0.01, 0.99)
        for batch in loader:
            img, mask, distmap, _, _ = create_combined_batch(batch) if isinstance(batch, dict) else batch
            if to_device:
                img, mask = img.to(to_device), mask.to(to_device)
                distmap = distmap.to(to_device) if distmap is not None else None
            loss = trainer.step(img, mask, distmap, alpha=alpha)
            # a replayed step hands back the graph's static output, the same tensor every time: the epoch mean needs a
            # copy of each value (without it the mean of replayed steps was the last step's loss)
            losses.append(loss.clone() if getattr(trainer, "use_graph", False) else loss)
        mean = float(torch.stack(losses).mean()) if losses else float("nan")
        history.append({"epoch": epoch, "lr": trainer.opt.lr, "train/total_loss": mean})
        if swa is not None:
            if epoch >= swa.swa_start:
                trainer.update_average()
            history[-1]["swa/n_averaged"] = trainer.averager.n_averaged
        stop = False
        if val_loader is not None and (epoch + 1) % check_val_every_n_epoch == 0:
            asked = dict(curves=True) if curves else {}
            if objects is not None:
                asked["objects"] = objects
            val = trainer.validate(val_loader, to_device=to_device, alpha=alpha, **asked)
            history[-1].update({k: v for k, v in val.items() if not k.startswith("cm_") and k not in ("curves", "objects")})
            if curves:
                history[-1].update(val["curves"].summary("val"))
            if objects is not None:
                crowns = val["objects"].summary("val")
                history[-1].update(crowns)
                val = {**val, **crowns}                          # what a crown-level monitor reads
            if select is not None:
                stop = select.update(epoch, val)
        if state is not None and (epoch + 1) % state.every_n_epochs == 0:
            from .utils.train_state import save_training_state
            save_training_state(state.path, trainer, {
                "epoch": epoch, "history": history, "sched": dict(sched), "swa_from": swa_from, "swa": _swa_record(swa),
                "base_lr": float(base_lr), "t_max": int(t_max), "stopped": bool(stop),
                "selection": None if select is None else select.state_dict(),
                "loader_next_epoch": int(getattr(loader, "_next_epoch", epoch + 1))},
                pl_module=pl_module, training_conf={"learning_rate": base_lr, "cosineannealing_tmax": t_max})
        if on_epoch_end:
            on_epoch_end(history[-1])
        if stop:
            break
    if swa is not None:
        trainer.swap_in_average()
        history.append({"swa/bn_batches": trainer.update_bn(loader, to_device=to_device)})
    if checkpoint is not None:
        history.append({"checkpoint/best_model_path": select.best_model_path,
                        "checkpoint/best_model_score": select.best_model_score})
    return history
