"""Exact resume, host side: ``ModelSelection``'s state through JSON, the state file (``weights_only`` reader, atomic write,
format check) and the argument validation of ``fit(state=..., resume=...)``.  No GPU."""
import json
import math
import os

import pytest
import torch

# val/dice (the checkpoint's monitor): finite values, a tie (epoch 2 == epoch 1), a NaN, a late best (epoch 6);
# val/total_loss (early stopping's, mode min): a tie, four epochs of waiting, then an improvement (epoch 6)
DICE = [0.50, 0.60, 0.60, 0.55, float("nan"), 0.58, 0.70, 0.65]
LOSS = [1.00, 0.90, 0.90, 0.95, 0.93, 0.92, 0.80, 0.85]
METRICS = [{"val/dice": d, "val/total_loss": l} for d, l in zip(DICE, LOSS)]


def _selection(tmp_path, calls, top_k=2, patience=10):
    from deadtrees_amd.trainer import CheckpointConfig, EarlyStoppingConfig, ModelSelection

    def save(path):
        calls.append(("save", os.path.basename(path)))
        with open(path, "w") as f:
            f.write("x")
    ck = CheckpointConfig(str(tmp_path), save_top_k=top_k)
    es = None if patience is None else EarlyStoppingConfig(monitor="val/total_loss", mode="min", patience=patience)
    return ModelSelection(ck, es, save)


def _run(tmp_path, metrics, round_trip_after=None, **kw):
    """-> (calls incl. the files present after every update, final selection, stop flags)"""
    calls, stops = [], []
    sel = _selection(tmp_path, calls, **kw)
    for epoch, v in enumerate(metrics):
        stops.append(sel.update(epoch, v))
        calls.append(("files", tuple(sorted(os.listdir(tmp_path)))))     # (a delete shows as a file gone)
        if stops[-1]:
            break
        if round_trip_after is not None and epoch + 1 == round_trip_after:
            text = json.dumps(sel.state_dict())
            sel = _selection(tmp_path, calls, **kw)
            sel.load_state_dict(json.loads(text))
    return calls, sel, stops


@pytest.mark.parametrize("kw", [dict(top_k=2, patience=10), dict(top_k=1, patience=5), dict(top_k=2, patience=4),
                                dict(top_k=1, patience=None)])
def test_model_selection_continues_through_json(tmp_path, kw):
    a, b = tmp_path / "direct", tmp_path / "resumed"
    a.mkdir()
    b.mkdir()
    calls_a, sel_a, stops_a = _run(a, METRICS, **kw)
    calls_b, sel_b, stops_b = _run(b, METRICS, round_trip_after=4, **kw)
    assert calls_a == calls_b
    assert stops_a == stops_b
    rel = lambda sel: [(s, os.path.basename(p)) for s, p in sel.kept]     # noqa: E731
    assert rel(sel_a) == rel(sel_b) and len(rel(sel_a)) == kw["top_k"]
    assert (sel_a.wait, sel_a.es_best, sel_a.stopped_epoch) == (sel_b.wait, sel_b.es_best, sel_b.stopped_epoch)
    assert sel_a.best_model_score == sel_b.best_model_score
    assert os.path.basename(sel_a.best_model_path) == os.path.basename(sel_b.best_model_path)


@pytest.mark.parametrize("mode,start", [("max", -math.inf), ("min", math.inf)])
def test_model_selection_es_best_still_infinite_at_the_round_trip(tmp_path, mode, start):
    """the round trip happens before any validated epoch: es_best is +-inf in the JSON text and comes back as that float"""
    from deadtrees_amd.trainer import EarlyStoppingConfig, ModelSelection
    sel = ModelSelection(None, EarlyStoppingConfig(monitor="val/total_loss" if mode == "min" else "val/dice", mode=mode,
                                                   patience=3), save=lambda p: None)
    assert sel.es_best == start
    text = json.dumps(sel.state_dict())
    assert "Infinity" in text
    sel2 = ModelSelection(None, sel.es, save=lambda p: None)
    sel2.load_state_dict(json.loads(text))
    assert sel2.es_best == start and sel2.wait == 0 and sel2.stopped_epoch is None and sel2.kept == []
    key = sel.es.monitor
    seq = [0.5, 0.4, 0.6, 0.6, 0.6, 0.6]
    assert [sel.update(e, {key: v}) for e, v in enumerate(seq)] == [sel2.update(e, {key: v}) for e, v in enumerate(seq)]
    assert (sel.wait, sel.es_best, sel.stopped_epoch) == (sel2.wait, sel2.es_best, sel2.stopped_epoch)


# ---------------------------------------------------------------------------------------------------- the file
def _trainer_state(n=24, segments=True, average=True, seed=0):
    g = torch.Generator().manual_seed(seed)
    opt = {"m": torch.randn(n, generator=g), "v": torch.rand(n, generator=g),
           "t_dev": torch.tensor([5.0], dtype=torch.float64), "hyper": torch.rand(3, generator=g),
           "lr_dev": torch.tensor([2.5e-4], dtype=torch.float64), "t": 7, "lr": 2.5e-4, "betas": [0.9, 0.999], "eps": 1e-8,
           "max_norm": 0.5, "_segments": None, "_trainable": None}
    if segments:
        opt.update(t_seg=torch.tensor([0.0, 5.0], dtype=torch.float64), hyper_seg=torch.rand(6, generator=g),
                   _segments=[[0, 8], [8, n]], _trainable=[False, True])
    return {"description": {"decoder": "unet", "in_channels": 3, "classes": 2, "n_params": n, "layout": "ab" * 32,
                            "precision": "bf16", "losses": ["GDICE", "FOCAL"], "average": "ema" if average else None,
                            "average_decay": 0.99 if average else None, "world": 1},
            "flat_params": torch.randn(n, generator=g), "bn_state": torch.randn(10, generator=g),
            "num_batches_tracked": torch.arange(4, dtype=torch.int64),
            "opt": opt,
            "averager": {"mode": "ema", "decay": 0.99, "avg": torch.randn(n, generator=g), "n_averaged": 6} if average else None,
            "flags": {"encoder_frozen": True, "encoder_training": False, "training": True}}


def _fit_state():
    return {"epoch": 2, "history": [{"epoch": e, "lr": 3e-4 / (e + 1), "train/total_loss": 0.1 * (e + 1) / 3} for e in range(3)],
            "sched": {"base_lr": 1e-4, "t_max": 10, "start": 2}, "swa_from": None, "swa": None, "base_lr": 3e-4, "t_max": 10,
            "stopped": False, "loader_next_epoch": 3,
            "selection": {"kept": [[0.5, "ck/epoch_001.ckpt"]], "best_model_path": "ck/epoch_001.ckpt",
                          "best_model_score": 0.5, "last_model_path": "ck/last.ckpt", "es_best": -math.inf, "wait": 1,
                          "stopped_epoch": None}}


def _assert_same(a, b, where=""):
    assert type(a) is type(b) or (isinstance(a, (list, tuple)) and isinstance(b, (list, tuple))), (where, a, b)
    if isinstance(a, dict):
        assert set(a) == set(b), where
        for k in a:
            _assert_same(a[k], b[k], f"{where}/{k}")
    elif isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and torch.equal(a, b), where
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _assert_same(x, y, f"{where}[{i}]")
    else:
        assert a == b, (where, a, b)


@pytest.mark.parametrize("segments,average", [(True, True), (False, False)])
def test_state_file_round_trip_weights_only(tmp_path, segments, average):
    from deadtrees_amd.utils.train_state import FORMAT, load_training_state, save_training_state
    tr, fs = _trainer_state(segments=segments, average=average), _fit_state()
    path = tmp_path / "state.pt"
    assert save_training_state(path, tr, fs) is True
    assert sorted(os.listdir(tmp_path)) == ["state.pt"]                   # no .tmp left behind
    flat = torch.load(str(path), map_location="cpu", weights_only=True)   # the restricted loader reads the file as it is
    assert flat["format"] == FORMAT
    for k, v in flat.items():     # a flat dict of tensors and JSON strings (and the format integer)
        assert isinstance(v, torch.Tensor) or (isinstance(v, str) and json.loads(v) is not None) or k == "format", k
    back = load_training_state(path)
    assert back["format"] == FORMAT
    _assert_same(back["trainer"], tr, "trainer")
    _assert_same(back["fit"], fs, "fit")
    assert back["fit"]["selection"]["es_best"] == -math.inf


def test_state_file_write_is_atomic(tmp_path, monkeypatch):
    from deadtrees_amd.utils.train_state import load_training_state, save_training_state
    path = tmp_path / "state.pt"
    save_training_state(path, _trainer_state(seed=1), _fit_state())
    before = path.read_bytes()
    real_save = torch.save

    def failing_save(obj, f, *a, **k):
        real_save({"half": torch.zeros(3)}, f)         # something is on disk when the write dies
        raise OSError("disk full")
    monkeypatch.setattr(torch, "save", failing_save)
    with pytest.raises(OSError, match="disk full"):
        save_training_state(path, _trainer_state(seed=2), _fit_state())
    monkeypatch.undo()
    assert sorted(os.listdir(tmp_path)) == ["state.pt"]
    assert path.read_bytes() == before
    _assert_same(load_training_state(path)["trainer"], _trainer_state(seed=1), "trainer")


def test_state_file_refuses_unknown_format_and_files_without_state(tmp_path):
    from deadtrees_amd.utils.train_state import FORMAT, load_training_state, pack_training_state
    flat = pack_training_state(_trainer_state(), _fit_state())
    flat["format"] = FORMAT + 1
    torch.save(flat, str(tmp_path / "future.pt"))
    with pytest.raises(ValueError, match="format"):
        load_training_state(tmp_path / "future.pt")
    # what checkpoint_writer writes: weights and hyper-parameters only
    torch.save({"state_dict": {"model.x": torch.zeros(2)}, "hyper_parameters_json": "{}"}, str(tmp_path / "last.ckpt"))
    with pytest.raises(ValueError, match="training state"):
        load_training_state(tmp_path / "last.ckpt")
    del flat["fit_json"]
    flat["format"] = FORMAT
    torch.save(flat, str(tmp_path / "partial.pt"))
    with pytest.raises(ValueError, match="training state"):
        load_training_state(tmp_path / "partial.pt")


# ---------------------------------------------------------------------------------------------------- fit's arguments
class _Untouchable:
    """a trainer none of whose attributes may be read: argument validation comes before anything runs"""

    def __getattr__(self, name):
        raise AssertionError(f"fit touched trainer.{name} before it had checked its arguments")


@pytest.mark.parametrize("kw,match", [
    (dict(state=3), "state"),
    (dict(state=""), "path"),
    (dict(state=("a", 1)), "state"),
    (dict(resume=7), "resume"),
    (dict(resume=""), "resume"),
    (dict(resume_overrides=True), "resume_overrides"),
    (dict(resume="x.pt", resume_overrides=1), "resume_overrides"),
])
def test_fit_validates_state_and_resume_before_anything_runs(kw, match):
    from deadtrees_amd.trainer import fit
    with pytest.raises(ValueError, match=match):
        fit(_Untouchable(), [], epochs=2, **kw)


@pytest.mark.parametrize("n", [0, -1, 1.5, True, "2", None])
def test_state_config_every_n_epochs(n):
    from deadtrees_amd.trainer import StateConfig, fit, resolve_state
    with pytest.raises(ValueError, match="every_n_epochs"):
        resolve_state(StateConfig("s.pt", every_n_epochs=n))
    with pytest.raises(ValueError, match="every_n_epochs"):
        fit(_Untouchable(), [], epochs=2, state=StateConfig("s.pt", every_n_epochs=n))


def test_state_config_resolves(tmp_path):
    from deadtrees_amd.trainer import StateConfig, resolve_state
    assert resolve_state(None) is None
    assert resolve_state("a/b.pt") == StateConfig("a/b.pt", 1)
    assert resolve_state(tmp_path / "s.pt") == StateConfig(str(tmp_path / "s.pt"), 1)
    assert resolve_state(StateConfig(tmp_path / "s.pt", 3)) == StateConfig(str(tmp_path / "s.pt"), 3)
    with pytest.raises(ValueError, match="path"):
        resolve_state(StateConfig(None))


def test_resume_of_a_missing_or_weights_only_file_touches_no_trainer(tmp_path):
    from deadtrees_amd.trainer import fit
    torch.save({"state_dict": {"model.x": torch.zeros(2)}, "hyper_parameters_json": "{}"}, str(tmp_path / "last.ckpt"))
    with pytest.raises(ValueError, match="training state"):
        fit(_Untouchable(), [], epochs=2, resume=tmp_path / "last.ckpt")
    with pytest.raises(FileNotFoundError):
        fit(_Untouchable(), [], epochs=2, resume=tmp_path / "nothing.pt")
