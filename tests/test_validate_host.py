"""Host side of validation in the trainer (no GPU): the checkpoint / early-stopping configurations, the selection rules
of ``ModelSelection`` on scripted scores with a stub writer, the batch-size weighted epoch mean, and the argument checks
``dt_head_eval`` makes before any launch."""
import ctypes
import math
import os

import pytest
import torch

from deadtrees_amd.trainer import (CheckpointConfig, EarlyStoppingConfig, ModelSelection, epoch_metrics,
                                   resolve_checkpoint, resolve_early_stopping, validation_keys)

LOSSES = ("GDICE", "FOCAL")


# ---------------------------------------------------------------------------------------------- configurations
def test_defaults_are_the_reference_callbacks(tmp_path):
    ck = resolve_checkpoint(CheckpointConfig(str(tmp_path)), LOSSES)
    assert (ck.monitor, ck.mode, ck.save_top_k, ck.save_last) == ("val/dice", "max", 1, True)
    assert ck.filename.format(epoch=7) == "epoch_007"
    es = resolve_early_stopping(EarlyStoppingConfig(), LOSSES)
    assert (es.monitor, es.mode, es.patience, es.min_delta) == ("val/dice", "max", 200, 0.0)
    assert resolve_checkpoint(None, LOSSES) is None and resolve_early_stopping(None, LOSSES) is None


def test_config_validation(tmp_path):
    d = str(tmp_path)
    with pytest.raises(ValueError, match="mode"):
        resolve_checkpoint(CheckpointConfig(d, mode="best"), LOSSES)
    with pytest.raises(ValueError, match="mode"):
        resolve_early_stopping(EarlyStoppingConfig(mode="up"), LOSSES)
    with pytest.raises(ValueError, match="patience"):
        resolve_early_stopping(EarlyStoppingConfig(patience=-1), LOSSES)
    with pytest.raises(ValueError, match="save_top_k"):
        resolve_checkpoint(CheckpointConfig(d, save_top_k=-1), LOSSES)
    with pytest.raises(ValueError, match="min_delta"):
        resolve_early_stopping(EarlyStoppingConfig(min_delta=-0.1), LOSSES)
    # a monitor the validation does not produce: a key of another stage, a term that is not enabled, a count
    for bad in ("train/dice", "val/boundary_loss", "val/iou", "val/samples"):
        with pytest.raises(ValueError, match="monitor"):
            resolve_checkpoint(CheckpointConfig(d, monitor=bad), LOSSES)
        with pytest.raises(ValueError, match="monitor"):
            resolve_early_stopping(EarlyStoppingConfig(monitor=bad), LOSSES)
    # ... which IS produced once the term is on
    assert resolve_early_stopping(EarlyStoppingConfig(monitor="val/boundary_loss", mode="min"),
                                  ("GDICE", "BOUNDARY")).monitor == "val/boundary_loss"
    with pytest.raises(ValueError):
        resolve_checkpoint({"dirpath": d}, LOSSES)
    with pytest.raises(ValueError, match="filename"):
        resolve_checkpoint(CheckpointConfig(d, filename="last"), LOSSES)
    with pytest.raises(ValueError, match="filename"):
        resolve_checkpoint(CheckpointConfig(d, filename="{step}"), LOSSES)


def test_validation_keys_follow_the_loss_list():
    assert validation_keys(LOSSES) == ("val/total_loss", "val/dice_loss", "val/dice", "val/dice_with_bg",
                                       "val/focal_loss", "val/batches", "val/samples")
    assert "test/boundary_loss" in validation_keys(("DICE", "BOUNDARY-RAMPED"), "test")
    assert "val/focal_loss" not in validation_keys(("GDICE",))


def test_fit_rejects_monitors_without_a_validation_loader(tmp_path):
    from deadtrees_amd.trainer import fit
    tr = type("T", (), {"losses": LOSSES, "world": 1})()
    with pytest.raises(ValueError, match="val_loader"):
        fit(tr, [], 1, checkpoint=CheckpointConfig(str(tmp_path)))
    with pytest.raises(ValueError, match="check_val_every_n_epoch"):
        fit(tr, [], 1, check_val_every_n_epoch=0)


# ---------------------------------------------------------------------------------------------- selection
def _drive(scores, ck=None, es=None, key="val/dice"):
    """the loop of ``fit`` on scripted scores; the stub writer records and writes one small file per call"""
    writes = []

    def save(path):
        writes.append(os.path.basename(path))
        with open(path, "w") as f:
            f.write("x")

    sel = ModelSelection(ck, es, save)
    ran = []
    for epoch, s in enumerate(scores):
        ran.append(epoch)
        if sel.update(epoch, {key: s}):
            break
    return sel, ran, writes


def test_selection_on_the_scripted_sequence(tmp_path):
    ck = resolve_checkpoint(CheckpointConfig(str(tmp_path)), LOSSES)
    es = resolve_early_stopping(EarlyStoppingConfig(patience=2), LOSSES)
    sel, ran, writes = _drive([0.5, 0.6, 0.6, 0.55, 0.7], ck, es)
    assert ran == [0, 1, 2, 3] and sel.stopped_epoch == 3          # epoch 4 never runs
    assert os.path.basename(sel.best_model_path) == "epoch_001.ckpt" and sel.best_model_score == 0.6
    assert sorted(os.listdir(tmp_path)) == ["epoch_001.ckpt", "last.ckpt"]     # the tie at epoch 2 replaced nothing
    assert writes == ["epoch_000.ckpt", "last.ckpt", "epoch_001.ckpt", "last.ckpt", "last.ckpt", "last.ckpt"]


def test_top_k_keeps_the_k_best_and_deletes_the_rest(tmp_path):
    ck = resolve_checkpoint(CheckpointConfig(str(tmp_path), save_top_k=2, save_last=False), LOSSES)
    sel, ran, _ = _drive([0.3, 0.1, 0.2, 0.2, 0.5], ck)
    assert ran == [0, 1, 2, 3, 4]
    assert sorted(os.listdir(tmp_path)) == ["epoch_000.ckpt", "epoch_004.ckpt"]
    assert os.path.basename(sel.best_model_path) == "epoch_004.ckpt" and sel.best_model_score == 0.5
    # save_top_k = 0: only last.ckpt
    d0 = tmp_path / "k0"
    sel, _, _ = _drive([0.3, 0.4], resolve_checkpoint(CheckpointConfig(str(d0), save_top_k=0), LOSSES))
    assert os.listdir(d0) == ["last.ckpt"] and sel.best_model_path is None


def test_mode_min_and_min_delta(tmp_path):
    ck = resolve_checkpoint(CheckpointConfig(str(tmp_path), monitor="val/total_loss", mode="min"), LOSSES)
    es = resolve_early_stopping(EarlyStoppingConfig(monitor="val/total_loss", mode="min", patience=2, min_delta=0.05), LOSSES)
    # 1.0 -> 0.9 improves; 0.86 is better but not by min_delta (wait 1); 0.84 improves on 0.9 by 0.06; then two misses
    sel, ran, _ = _drive([1.0, 0.9, 0.86, 0.84, 0.83, 0.80, 0.1], ck, es, key="val/total_loss")
    assert ran == [0, 1, 2, 3, 4, 5] and sel.stopped_epoch == 5
    assert sel.es_best == 0.84
    # the checkpoint has no min_delta: the strictly smallest score seen is kept
    assert os.path.basename(sel.best_model_path) == "epoch_005.ckpt" and sel.best_model_score == 0.80
    assert sorted(os.listdir(tmp_path)) == ["epoch_005.ckpt", "last.ckpt"]
    # mode max with min_delta
    es = resolve_early_stopping(EarlyStoppingConfig(patience=1, min_delta=0.1), LOSSES)
    sel, ran, _ = _drive([0.5, 0.55, 0.9], None, es)
    assert ran == [0, 1] and sel.es_best == 0.5


def test_patience_zero_and_non_finite_scores(tmp_path):
    es = resolve_early_stopping(EarlyStoppingConfig(patience=0), LOSSES)
    _, ran, _ = _drive([0.5, 0.6, 0.6, 0.9], None, es)
    assert ran == [0, 1, 2]
    ck = resolve_checkpoint(CheckpointConfig(str(tmp_path)), LOSSES)
    es = resolve_early_stopping(EarlyStoppingConfig(patience=50), LOSSES)
    for bad in (float("nan"), float("inf")):
        sel, ran, _ = _drive([0.5, bad, 0.9], ck, es)
        assert ran == [0, 1] and sel.stopped_epoch == 1              # a non-finite monitored value stops training
        assert os.path.basename(sel.best_model_path) == "epoch_000.ckpt"    # and is never kept as a best file
        assert sorted(os.listdir(tmp_path)) == ["epoch_000.ckpt", "last.ckpt"]
    with pytest.raises(KeyError):
        ModelSelection(None, es, lambda p: None).update(0, {"val/total_loss": 1.0})


def test_ranks_other_than_zero_decide_without_writing(tmp_path):
    d = tmp_path / "none"
    ck = resolve_checkpoint(CheckpointConfig(str(d)), LOSSES)
    es = resolve_early_stopping(EarlyStoppingConfig(patience=2), LOSSES)
    sel = ModelSelection(ck, es, lambda p: pytest.fail("wrote a file"), write=False)
    stops = [sel.update(e, {"val/dice": s}) for e, s in enumerate([0.5, 0.6, 0.6, 0.55])]
    assert stops == [False, False, False, True] and not d.exists()
    assert os.path.basename(sel.best_model_path) == "epoch_001.ckpt"


# ---------------------------------------------------------------------------------------------- weighted mean
def test_epoch_values_are_batch_size_weighted_means():
    """three batches of sizes 4, 2, 1: the epoch buffer holds sum_b w_b parts_b and sum_b w_b"""
    parts = torch.tensor([[0.40, 0.0, 0.10, 0.3, 0.70, 0.80, 0.50, 0.50],
                          [0.20, 0.0, 0.30, 0.3, 0.90, 0.95, 0.50, 0.50],
                          [0.90, 0.0, 0.60, 0.3, 0.10, 0.55, 1.50, 1.50]], dtype=torch.float64)
    w = torch.tensor([4.0, 2.0, 1.0], dtype=torch.float64)
    epoch = torch.cat([(w[:, None] * parts).sum(0), w.sum()[None]])
    counts = torch.tensor([[[5, 1], [2, 0]], [[3, 0], [0, 0]]])
    out = epoch_metrics(epoch, counts, LOSSES, "val", 3)
    assert out["val/dice"] == pytest.approx((4 * 0.7 + 2 * 0.9 + 0.1) / 7, rel=1e-15)
    assert out["val/dice"] != pytest.approx((0.7 + 0.9 + 0.1) / 3, rel=1e-3)        # not the plain mean
    assert out["val/dice_with_bg"] == pytest.approx((4 * 0.8 + 2 * 0.95 + 0.55) / 7, rel=1e-15)
    assert out["val/dice_loss"] == pytest.approx((4 * 0.4 + 2 * 0.2 + 0.9) / 7, rel=1e-15)
    assert out["val/focal_loss"] == pytest.approx((4 * 0.1 + 2 * 0.3 + 0.6) / 7, rel=1e-15)
    assert out["val/total_loss"] == pytest.approx((4 * 0.5 + 2 * 0.5 + 1.5) / 7, rel=1e-15)
    assert out["val/batches"] == 3.0 and out["val/samples"] == 7.0
    assert "val/boundary_loss" not in out
    assert set(k for k in out if k.startswith("val/")) == set(validation_keys(LOSSES))
    assert all(isinstance(out[k], float) for k in validation_keys(LOSSES))
    # the matrices of SemSegment.confusion_matrices: rows normalised, an empty row stays zero
    assert out["cm_px"].dtype == torch.int64 and out["cm_px"].tolist() == [[5, 1], [2, 0]]
    assert out["cm_norm"].tolist() == [[5 / 6, 1 / 6], [1.0, 0.0]]
    assert out["cm_px_masked"].tolist() == [[3, 0], [0, 0]] and out["cm_norm_masked"].tolist() == [[1.0, 0.0], [0.0, 0.0]]
    with pytest.raises(ValueError):
        epoch_metrics(torch.zeros(9), counts, LOSSES, "val", 0)


# ---------------------------------------------------------------------------------------------- C ABI, host side
def test_head_eval_rejects_bad_arguments_before_any_launch():
    import __graft_entry__ as g
    g.build()
    from deadtrees_amd import _lib
    lib = _lib.load()
    p = 0x1000          # never dereferenced: every call below is refused on the host
    B, H, W = 1, 8, 32

    def call(fn, x=p, w=p, bias=p, labels=p, acc=p, counts=p, err=p, Cin=16, K=2, B=B):
        return fn(x, w, bias, labels, None, None, 2.0, acc, counts, None, err, B, H, W, Cin, K, None)

    for fn in (lib.dt_head_eval, lib.dt_head_eval_bf16):
        assert call(fn, Cin=32) != 0
        assert b"Cin" in lib.dt_last_error()
        for K in (5, 1):
            assert call(fn, K=K) != 0
            assert f"K={K}".encode() in lib.dt_last_error()
        for name in ("x", "w", "bias", "labels", "acc", "counts", "err"):
            assert call(fn, **{name: None}) != 0, name
            assert b"null" in lib.dt_last_error()
        assert call(fn, B=0) != 0
        assert b"sizes" in lib.dt_last_error()
    assert lib.dt_eval_accumulate(None, 1.0, p, None) != 0 and b"null" in lib.dt_last_error()
    assert lib.dt_eval_accumulate(p, -1.0, p, None) != 0 and b"weight" in lib.dt_last_error()
    # the accumulator: [B][K][10] results + one [K][10] row per 16 tiles (8 x 32 pixels each) of an image
    assert lib.dt_head_eval_acc_doubles(2, 2, 8, 32) == 2 * (1 + 1) * 2 * 10
    assert lib.dt_head_eval_acc_doubles(2, 2, 72, 96) == 2 * (1 + 2) * 2 * 10          # 27 tiles: 16 + 11
    assert lib.dt_head_eval_acc_doubles(32, 2, 512, 512) == 32 * (1 + 64) * 2 * 10
    assert lib.dt_head_eval_acc_doubles(0, 2, 8, 32) == 0
    assert math.isfinite(lib.dt_version())
