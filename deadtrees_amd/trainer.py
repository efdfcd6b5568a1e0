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

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence

import torch

from .data.distmap import distmaps_on_device
from .loss.seg_loss import PART_KEYS, loss_backward, loss_forward
from .network.unet import UNetHIP
from .ops import FlatAdam, WeightAverager


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
        the Python launch path."""
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
        self._graph = None
        self.averager = None if average is None else WeightAverager(model.flat_params.data, average)
        self._recal_graph = None

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
        m, eng = self.model, self.model.engine
        key = (tuple(x.shape), precision)
        g = self._recal_graph
        if g is None or g["key"] != key:
            self._recal_graph = g = {"key": key, "warm": 0}
        if "graph" not in g:
            if g["warm"] < 2:    # eager warm-up: lazy initialisation (workspaces) must not be captured
                g["warm"] += 1
                return m.recalibrate_batch(x, precision)
            g["x"] = x.clone()
            graph = torch.cuda.CUDAGraph()
            with eng.capture_workspaces() as g["ws"]:   # workspaces of the captured pass live (and stay) in the graph's pool
                torch.cuda.synchronize()
                with torch.cuda.graph(graph):
                    m.recalibrate_batch(g["x"], precision)
            g["graph"] = graph
        if x is not g["x"]:
            g["x"].copy_(x)
        g["graph"].replay()

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
        g = self._graph
        if g is None or g["key"] != key:
            self._graph = g = {"key": key, "warm": 0}     # new shapes / loss blend: drop the old graph, warm up again
        if "graph" not in g:
            if g["warm"] < 2:    # eager warm-up: lazy initialisation (workspaces, autograd) must not be captured
                g["warm"] += 1
                return self._eager_step(img, mask, distmap, alpha)
            self._capture(g, img, mask, distmap, alpha)
        # a loader that writes its batches straight into the graph's static buffers (`static_batch()`) hands them back
        # here: nothing to copy (at B = 64 the image copy alone is 201 MB = 0.2 ms of a 25 ms step)
        if img is not g["img"]:
            g["img"].copy_(img)
        if mask is not g["mask"]:
            g["mask"].copy_(mask)
        if distmap is not None and distmap is not g["distmap"]:
            g["distmap"].copy_(distmap)
        self.opt.sync_lr()                   # a changed learning rate reaches the replay through lr_dev
        self.opt.t += 1                      # host mirror; the authoritative count is the device's t_dev
        g["graph"].replay()
        self.model.engine.mark_weights_changed()
        self.model._bn_tracked_inc()         # module bookkeeping outside the graph (smp state_dict key)
        self.last = g["last"]
        return g["last"]["loss"]

    def static_batch(self):
        """(img, mask, distmap) buffers the captured step reads — available once the graph exists (after the eager
        warm-up steps); a data pipeline that fills THESE tensors (H2D copies, device-side augmentation) and passes them
        to ``step`` saves the per-step staging copy.  None before capture or without graph replay."""
        g = self._graph
        if not self.use_graph or g is None or "graph" not in g:
            return None
        return g["img"], g["mask"], g["distmap"]

    def _capture(self, g, img, mask, distmap, alpha):
        eng = self.model.engine
        g["img"], g["mask"] = img.clone(), mask.clone()
        g["distmap"] = None if distmap is None else distmap.clone()
        self.opt.sync_lr()
        t_host = self.opt.t
        graph = torch.cuda.CUDAGraph()
        with eng.capture_workspaces() as g["ws"]:   # workspaces of the captured step live (and stay) in the graph's pool
            torch.cuda.synchronize()
            with torch.cuda.graph(graph):
                self._eager_step(g["img"], g["mask"], g["distmap"], alpha, capturing=True)
        self.opt.t = t_host                   # capture launched nothing: the step count has not moved
        g["graph"], g["last"] = graph, self.last

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


def fit(trainer: HipTrainer, loader, epochs: int, base_lr: float = 3e-4, t_max: int = 10, to_device=None,
        on_epoch_end=None, callbacks=None, pl_module=None, swa=None):
    """Minimal stand-in for ``Trainer.fit`` on the hot path (reference deadtrees/train.py:113): per-batch
    ``HipTrainer.step`` and the per-epoch ``CosineAnnealingLR(T_max)`` of segmodel.py:426-428.

    callbacks: objects with ``on_train_epoch_start(trainer, pl_module)`` (e.g. ``MultiStage``), called at the start of
    every epoch with views of this trainer and of ``pl_module`` (a ``SemSegment``; default: a view of the trainer's model
    with ``encoder_weights`` taken from the model and ``hparams.training`` = learning_rate / cosineannealing_tmax).
    There is no validation loop here, so an encoder put in eval mode stays there (Lightning puts the whole module back
    in train mode after every validation run).

    swa: None | True | SWAConfig — the loop of torch's SWA documentation on a ``HipTrainer(average="swa")``: epochs before
    ``swa_start`` keep the cosine schedule (or whatever a callback put in its place); from ``swa_start`` the rate follows
    ``swa_lr`` (SWALR, annealing from the rate the schedule had reached) and the average is updated at the end of every
    epoch; after the last epoch the average is swapped in and the BatchNorm statistics are recomputed over ``loader``.
    The history then carries "swa/n_averaged" per epoch and a final {"swa/bn_batches": k} record."""
    from .network.segmodel import cosine_lr, create_combined_batch
    from .utils.config import to_attrdict
    swa = resolve_swa(swa, epochs, base_lr)
    if swa is not None and (getattr(trainer, "averager", None) is None or trainer.averager.mode != "swa"):
        raise ValueError("fit(swa=...) needs HipTrainer(average='swa')")
    swa_from = None       # the rate the schedule had reached when SWA took over
    history = []
    sched = {"base_lr": float(base_lr), "t_max": int(t_max), "start": 0}
    tview = _TrainerView(trainer, sched)
    if callbacks and pl_module is None:
        hp = to_attrdict({"training": {"learning_rate": base_lr, "cosineannealing_tmax": t_max}})
        pl_module = _ModuleView(trainer.model, getattr(trainer.model, "encoder_weights", None), hp)
    elif callbacks and not hasattr(pl_module, "model"):
        raise ValueError("fit(callbacks=...): pl_module must have .model")
    for epoch in range(epochs):
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
        for batch in loader:
            img, mask, distmap, _, _ = create_combined_batch(batch) if isinstance(batch, dict) else batch
            if to_device:
                img, mask = img.to(to_device), mask.to(to_device)
                distmap = distmap.to(to_device) if distmap is not None else None
            alpha = min((epoch + 1) * 0.01, 0.99)
            losses.append(trainer.step(img, mask, distmap, alpha=alpha))
        mean = float(torch.stack(losses).mean()) if losses else float("nan")
        history.append({"epoch": epoch, "lr": trainer.opt.lr, "train/total_loss": mean})
        if swa is not None:
            if epoch >= swa.swa_start:
                trainer.update_average()
            history[-1]["swa/n_averaged"] = trainer.averager.n_averaged
        if on_epoch_end:
            on_epoch_end(history[-1])
    if swa is not None:
        trainer.swap_in_average()
        history.append({"swa/bn_batches": trainer.update_bn(loader, to_device=to_device)})
    return history
