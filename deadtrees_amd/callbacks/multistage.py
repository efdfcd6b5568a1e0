"""``MultiStage`` — the staged fine-tuning callback of the reference's default recipe (configs/callbacks/default.yaml:
unfreeze_epoch 20, lr_reduce_epoch 40, lr_reduce_fraction 3), for ``deadtrees_amd.trainer.fit(callbacks=[...])`` or a
Lightning trainer.

Same stages as the reference (deadtrees/callbacks/multistage.py):
  epoch 0              exit() without encoder weights; otherwise ``model.encoder.eval()`` (the encoder's BatchNorm on
                       its running statistics) and ``m.requires_grad_ = False`` on every encoder module — an attribute
                       assignment, not a call, so the encoder's weights keep training (as in the reference)
  unfreeze_epoch       ``model.encoder.train()``
  lr_reduce_epoch      a fresh Adam with lr = learning_rate / lr_reduce_fraction and a fresh CosineAnnealingLR
One opt-in addition: ``freeze_weights=True`` also calls ``model.encoder.requires_grad_(False)`` at epoch 0 (and
``requires_grad_(True)`` at unfreeze_epoch) — what the reference's author evidently intended; the frozen step computes
no encoder gradient at all.
"""
from __future__ import annotations

import logging
import sys
from typing import Optional

import torch

log = logging.getLogger(__name__)


class MultiStage:
    def __init__(self, *, unfreeze_epoch: int, lr_reduce_epoch: Optional[int] = None,
                 lr_reduce_fraction: Optional[float] = None, freeze_weights: bool = False):
        self.unfreeze_epoch = unfreeze_epoch          # epoch when to unfreeze encoder
        self.lr_reduce_epoch = lr_reduce_epoch        # epoch when to reduce learning rate
        self.lr_reduce_fraction = lr_reduce_fraction  # reduce learning rate by fraction
        self.freeze_weights = bool(freeze_weights)

    def on_train_epoch_start(self, trainer, pl_module):
        if trainer.current_epoch == 0:
            if pl_module.encoder_weights is None:
                log.error("No encoder weights given but MultiStage encoder freeze requested")
                sys.exit()      # the reference's exit(): the same SystemExit, without closing sys.stdin
            log.info(f"Using pre-trained encoder weights: {pl_module.encoder_weights}")
            log.info(f"NEW STAGE (epoch: {trainer.current_epoch}): Freeze encoder")
            pl_module.model.encoder.eval()
            if self.freeze_weights:
                pl_module.model.encoder.requires_grad_(False)
            for m in pl_module.model.encoder.modules():
                m.requires_grad_ = False

        if trainer.current_epoch == self.unfreeze_epoch:
            log.info(f"NEW STAGE (epoch: {trainer.current_epoch}): Unfreeze encoder")
            pl_module.model.encoder.train()
            if self.freeze_weights:
                pl_module.model.encoder.requires_grad_(True)
            for m in pl_module.model.encoder.modules():
                m.requires_grad_ = True

        if self.lr_reduce_epoch:
            assert self.lr_reduce_fraction is not None     # a reduce epoch needs a fraction
            if trainer.current_epoch == self.lr_reduce_epoch:
                log.info(f"NEW STAGE (epoch: {trainer.current_epoch}): Lower LR rate by factor {self.lr_reduce_fraction}")
                new_optimizer = torch.optim.Adam(pl_module.parameters(),
                                                 lr=pl_module.hparams.training.learning_rate / self.lr_reduce_fraction)
                new_scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(
                    new_optimizer, T_max=pl_module.hparams.training.cosineannealing_tmax)
                trainer.optimizers = [new_optimizer]
                trainer.lr_schedulers = trainer._configure_schedulers([new_scheduler], monitor=None,
                                                                      is_manual_optimization=False)
                trainer.optimizer_frequencies = []
