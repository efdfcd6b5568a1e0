"""Exact resume on the MI355X: ``fit(state=...)`` / ``fit(resume=...)`` against the uninterrupted run under ``torch.equal``,
its controls, restore under a captured graph, the refusals and the inference readers of a state file.  Needs an MI355X.

Sizes are those of ``test_swa_gpu.py``'s ``fit`` tests: B = 2, 64x64, C = 3, K = 2, two batches per epoch."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPOCHS, KILL_AFTER = 6, 2


class _Killed(Exception):
    """what run B's ``on_epoch_end`` raises: the run dies after the state of epoch ``KILL_AFTER`` was written"""


def _loader(seed=40):
    from deadtrees_amd.data.synthetic import synth_batch
    return [synth_batch(2, 64, 64, 3, 2, seed=seed + i) + (None, None, None) for i in range(2)]


def _val_loader():
    from deadtrees_amd.data.synthetic import synth_batch
    return [synth_batch(2, 64, 64, 3, 2, seed=70 + i) for i in range(2)]


def _model(decoder="unet", seed=0):
    from deadtrees_amd.network.unet import UNetHIP
    m = UNetHIP(in_channels=3, classes=2, decoder=decoder)
    m.reset_parameters(seed=seed)
    return m.to(DEV)


def _case(name):
    """-> (decoder, HipTrainer keywords, a function () -> fit keywords; fresh callback objects for every run)"""
    from deadtrees_amd.callbacks.multistage import MultiStage
    from deadtrees_amd.trainer import CheckpointConfig, EarlyStoppingConfig, SWAConfig
    if name == "fp32_eager":
        return "unet", {}, dict
    if name == "bf16_graph_ema":
        return "unet", dict(precision="bf16", graph=True, average=("ema", 0.99)), dict
    if name == "fp32_graph_swa":        # the interruption falls inside the SWA phase
        return "unet", dict(graph=True, average="swa"), lambda: dict(swa=SWAConfig(swa_start=2, swa_lr=1e-4, anneal_epochs=2))
    if name == "multistage_frozen":     # killed while the encoder is frozen, after the optimiser reset; resumed over the unfreeze
        return "unet", {}, lambda: dict(callbacks=[MultiStage(unfreeze_epoch=4, lr_reduce_epoch=2, lr_reduce_fraction=3,
                                                              freeze_weights=True)])
    if name == "resunet":               # a 1x1 head held as a 3x3 kernel: eight taps per weight that no smp key names
        return "resunet", {}, dict
    if name == "selection":             # (dirpath is relative: every run works in a directory of its own)
        return "unet", {}, lambda: dict(val_loader=_val_loader(), checkpoint=CheckpointConfig("ck", save_top_k=1),
                                        early_stopping=EarlyStoppingConfig(patience=10))
    raise KeyError(name)


CASES = ["fp32_eager", "bf16_graph_ema", "fp32_graph_swa", "multistage_frozen", "resunet", "selection"]


def _trainer(name, seed=0):
    from deadtrees_amd.trainer import HipTrainer
    decoder, tkw, fkw = _case(name)
    m = _model(decoder, seed)
    if name == "multistage_frozen":
        m.encoder_weights = "given"      # (the callback only asks whether there are any)
    return HipTrainer(m, **tkw), fkw


def _tensors(tr):
    m, opt = tr.model, tr.opt
    out = {"flat_params": m.flat_params.detach(), "bn_state": m.bn_state, "num_batches_tracked": m.num_batches_tracked,
           "opt.m": opt.m, "opt.v": opt.v, "opt.t_dev": opt.t_dev}
    if opt.t_seg is not None:
        out["opt.t_seg"] = opt.t_seg
    if tr.averager is not None:
        out["average"], out["average.count"] = tr.averager.avg, tr.averager.n_dev
    return out


def _snapshot(tr):
    return {k: v.clone() for k, v in _tensors(tr).items()}


def _fingerprint(tr):
    """an exact-equality fingerprint of every state tensor (the bit patterns summed as integers), cheap enough to take
    after every epoch"""
    out = {}
    for k, v in _tensors(tr).items():
        bits = v.contiguous().view(torch.int32 if v.element_size() == 4 else torch.int64)
        out[k] = int(bits.to(torch.int64).sum())
    return out


def _assert_equal_state(got, want, tag):
    assert set(got) == set(want), (tag, sorted(got), sorted(want))
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), f"{tag}: {k} differs"


def _run(name, state_path, seed=0, kill=False, resume=None):
    """one ``fit`` of case `name` -> dict(history, prints: {epoch: fingerprint}, at_kill: snapshot after epoch KILL_AFTER,
    final: snapshot after fit, steps, trainer)"""
    from deadtrees_amd.trainer import StateConfig, fit
    tr, fkw = _trainer(name, seed)
    out = {"prints": {}, "at_kill": None, "trainer": tr, "history": None}

    def on_epoch_end(rec):
        out["prints"][rec["epoch"]] = _fingerprint(tr)
        if rec["epoch"] == KILL_AFTER:
            out["at_kill"] = _snapshot(tr)
            if kill:
                raise _Killed()
    # (the state is some 0.4 GB: written after epochs 2 and 5 only, which is where the runs are killed and compared)
    kw = dict(epochs=EPOCHS, base_lr=3e-4, t_max=10, to_device=DEV, on_epoch_end=on_epoch_end,
              state=StateConfig(state_path, every_n_epochs=KILL_AFTER + 1), **fkw())
    if kill:
        with pytest.raises(_Killed):
            fit(tr, _loader(), resume=resume, **kw)
    else:
        out["history"] = fit(tr, _loader(), resume=resume, **kw)
    out["final"], out["steps"] = _snapshot(tr), tr.opt.steps_applied()
    return out


def _dir(tmp_path, monkeypatch, name):
    d = tmp_path / name
    d.mkdir(exist_ok=True)
    monkeypatch.chdir(d)
    return d


@pytest.fixture(scope="module")
def full_runs():
    """the uninterrupted run A of the cases more than one test needs (history, state at the kill epoch, final state)"""
    return {}


def _run_a(full_runs, name, tmp_path, monkeypatch):
    if name in full_runs:
        return full_runs[name]
    d = _dir(tmp_path, monkeypatch, "A")
    a = _run(name, str(d / "state.pt"))
    del a["trainer"]
    if name in ("fp32_eager", "bf16_graph_ema"):
        full_runs[name] = a
    return a


# -------------------------------------------------------------------------------------------- 1. exact continuation
@pytest.mark.parametrize("name", CASES)
def test_resumed_run_equals_the_uninterrupted_run(name, tmp_path, monkeypatch, full_runs):
    a = _run_a(full_runs, name, tmp_path, monkeypatch)
    d = _dir(tmp_path, monkeypatch, "B")
    path_b = str(d / "state.pt")
    b = _run(name, path_b, kill=True)
    # B died where A went on: equal there, or the step is not reproducible and nothing below means anything
    _assert_equal_state(b["at_kill"], a["at_kill"], f"{name}: run B at its kill (before any resume) vs run A")
    del b
    c = _run(name, str(d / "state_c.pt"), seed=99, resume=path_b)
    assert sorted(c["prints"]) == list(range(KILL_AFTER + 1, EPOCHS))
    for epoch in sorted(c["prints"]):
        assert c["prints"][epoch] == a["prints"][epoch], f"{name}: state after epoch {epoch} differs"
    _assert_equal_state(c["final"], a["final"], f"{name}: resumed vs uninterrupted, after fit")
    assert c["steps"] == a["steps"]
    assert len(c["history"]) == len(a["history"])
    for got, want in zip(c["history"], a["history"]):
        assert got == want, (name, got, want)
    assert [h["lr"] for h in c["history"] if "lr" in h] == [h["lr"] for h in a["history"] if "lr" in h]
    if name == "selection":
        sel_a = a["history"][-1]
        assert set(sel_a) == {"checkpoint/best_model_path", "checkpoint/best_model_score"} and c["history"][-1] == sel_a
        assert sorted(os.listdir(tmp_path / "A" / "ck")) == sorted(os.listdir(d / "ck"))
        from deadtrees_amd.utils.train_state import load_training_state
        end_a = load_training_state(tmp_path / "A" / "state.pt")["fit"]
        end_c = load_training_state(d / "state_c.pt")["fit"]
        assert end_a["epoch"] == end_c["epoch"] == EPOCHS - 1
        assert end_a["selection"] == end_c["selection"]
        assert end_a["selection"]["wait"] == end_c["selection"]["wait"]
    if name == "multistage_frozen":
        tr = c["trainer"]
        assert not tr.model.encoder_frozen and tr.model.encoder.training and "opt.t_seg" in c["final"]
        assert c["final"]["opt.t_seg"].tolist() == [4.0, 8.0]      # 2 epochs of 2 steps unfrozen; 4 since the reset
    if name == "fp32_graph_swa":
        assert c["history"][-1] == {"swa/bn_batches": 2} and c["history"][-2]["swa/n_averaged"] == 4
        assert torch.equal(c["final"]["flat_params"], c["final"]["average"])


# -------------------------------------------------------------------------------------------- 2. control
@pytest.mark.parametrize("name", ["fp32_eager", "bf16_graph_ema"])
def test_control_two_uninterrupted_runs_are_equal(name, tmp_path, monkeypatch, full_runs):
    a = _run_a(full_runs, name, tmp_path, monkeypatch)
    d = _dir(tmp_path, monkeypatch, "A2")
    a2 = _run(name, str(d / "state.pt"))
    why = f"{name}: two uninterrupted runs differ - the training step is not run-to-run reproducible (not a resume fault)"
    assert a2["prints"] == a["prints"], why
    _assert_equal_state(a2["final"], a["final"], why)
    assert a2["history"] == a["history"], why


# -------------------------------------------------------------------------------------------- 3. the test can tell
def test_a_restart_from_weights_alone_does_not_equal_the_uninterrupted_run(tmp_path, monkeypatch, full_runs):
    from deadtrees_amd.trainer import HipTrainer, fit
    from deadtrees_amd.utils.train_state import load_training_state
    a = _run_a(full_runs, "fp32_eager", tmp_path, monkeypatch)
    d = _dir(tmp_path, monkeypatch, "B")
    path_b = str(d / "state.pt")
    _run("fp32_eager", path_b, kill=True)
    m = _model(seed=99)
    m.load_smp_state_dict({k[len("model."):]: v for k, v in load_training_state(path_b)["state_dict"].items()})
    assert torch.equal(m.flat_params.detach(), a["at_kill"]["flat_params"])      # the weights ARE those of epoch 2
    tr = HipTrainer(m)
    fit(tr, _loader(), epochs=EPOCHS - KILL_AFTER - 1, base_lr=3e-4, t_max=10, to_device=DEV)
    assert tr.opt.steps_applied() == 2 * (EPOCHS - KILL_AFTER - 1)
    assert not torch.equal(m.flat_params.detach(), a["final"]["flat_params"])
    assert not torch.equal(tr.opt.m, a["final"]["opt.m"])


# -------------------------------------------------------------------------------------------- 4. under a captured graph
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_load_state_dict_under_a_captured_graph(precision):
    from deadtrees_amd.trainer import HipTrainer
    batches = [tuple(t.to(DEV) for t in b[:2]) for b in _loader(seed=10) + _loader(seed=20) + _loader(seed=30)]
    tr = HipTrainer(_model(), precision=precision, graph=True, average=("ema", 0.9))
    for img, mask in batches[:3]:
        tr.step(img, mask)
    assert tr.static_batch() is not None                  # two warm-up steps, then the capture
    ptrs = {k: v.data_ptr() for k, v in _tensors(tr).items()}
    sd = tr.state_dict()
    for img, mask in batches[3:5]:
        tr.step(img, mask)
    want = _snapshot(tr)
    assert not torch.equal(want["flat_params"], sd["flat_params"].to(DEV))
    tr.load_state_dict(sd)
    assert tr.static_batch() is None                      # the graph is gone: the next step warms up and captures again
    assert {k: v.data_ptr() for k, v in _tensors(tr).items()} == ptrs     # restored in place
    assert torch.equal(tr.model.flat_params.detach(), sd["flat_params"].to(DEV)) and tr.opt.steps_applied() == 3
    for img, mask in batches[3:5]:
        tr.step(img, mask)
    assert tr.static_batch() is None
    _assert_equal_state(_snapshot(tr), want, f"{precision}: two steps again after load_state_dict")
    tr.step(*batches[5])
    assert tr.static_batch() is not None and tr.opt.steps_applied() == 6


# -------------------------------------------------------------------------------------------- 5. refusals
@pytest.fixture(scope="module")
def target():
    """an fp32 trainer without average, one step in (so every tensor holds something), and a clone of its tensors"""
    from deadtrees_amd.trainer import HipTrainer
    tr = HipTrainer(_model(seed=5))
    img, mask = (t.to(DEV) for t in _loader()[0][:2])
    tr.step(img, mask)
    return tr, _snapshot(tr)


def _state_file(path, decoder="unet", epochs=1, fit_kw=None, **trainer_kw):
    from deadtrees_amd.trainer import HipTrainer, fit
    tr = HipTrainer(_model(decoder, seed=3), **trainer_kw)
    fit(tr, _loader(), epochs=epochs, to_device=DEV, state=str(path), **(fit_kw or {}))
    return tr


def _write_refused(kind, path):
    """-> (fit keywords of the resuming call, what the ValueError must say)"""
    from deadtrees_amd.trainer import EarlyStoppingConfig, HipTrainer, checkpoint_writer
    if kind == "bf16_into_fp32":
        _state_file(path, precision="bf16")
        return {}, "precision"
    if kind == "other_losses":
        _state_file(path, losses=("GDICE",))
        return {}, "losses"
    if kind == "other_decoder":
        _state_file(path, decoder="resunet")
        return {}, "decoder"
    if kind == "average_missing":
        _state_file(path, average=("ema", 0.99))
        return {}, "average"
    if kind == "weights_only":
        checkpoint_writer(HipTrainer(_model(seed=3)))(str(path))
        return {}, "training state"
    if kind == "finished":
        _state_file(path, epochs=2)
        return dict(epochs=2), "pass a larger epochs"
    if kind == "early_stopped":          # min_delta so large that only the first epoch improves: stopped after epoch 1
        es = EarlyStoppingConfig(patience=1, min_delta=1e9)
        _state_file(path, epochs=4, fit_kw=dict(val_loader=_val_loader(), early_stopping=es))
        return dict(val_loader=_val_loader(), early_stopping=es), "stopped"
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["bf16_into_fp32", "other_losses", "other_decoder", "average_missing", "weights_only",
                                  "finished", "early_stopped"])
def test_refused_resume_leaves_the_trainer_untouched(kind, tmp_path, target):
    from deadtrees_amd.trainer import fit
    tr, before = target
    path = tmp_path / "state.pt"
    fkw, says = _write_refused(kind, path)
    flags = (tr.model.training, tr.model.encoder.training, tr.model.encoder_frozen, tr.opt.t, tr.opt.lr)
    with pytest.raises(ValueError, match=says):
        fit(tr, _loader(), to_device=DEV, resume=str(path), **{"epochs": EPOCHS, **fkw})
    _assert_equal_state(_snapshot(tr), before, f"{kind}: refused, yet the trainer changed")
    assert flags == (tr.model.training, tr.model.encoder.training, tr.model.encoder_frozen, tr.opt.t, tr.opt.lr)
    assert sorted(os.listdir(tmp_path)) == ["state.pt"]


def test_refused_other_schedule_unless_overridden(tmp_path):
    from deadtrees_amd.trainer import SWAConfig, fit
    path = tmp_path / "state.pt"
    tr = _state_file(path, epochs=2, average="swa")
    before = _snapshot(tr)
    for kw, says in ((dict(base_lr=1e-4), "base_lr"), (dict(t_max=7), "t_max"),
                     (dict(swa=SWAConfig(swa_start=3)), "swa")):
        with pytest.raises(ValueError, match=says):
            fit(tr, _loader(), epochs=4, to_device=DEV, resume=str(path), **kw)
        _assert_equal_state(_snapshot(tr), before, f"{says}: refused, yet the trainer changed")
    from deadtrees_amd.network.segmodel import cosine_lr
    hist = fit(tr, _loader(), epochs=4, base_lr=1e-4, to_device=DEV, resume=str(path), resume_overrides=True)
    assert [h["epoch"] for h in hist] == [0, 1, 2, 3]
    assert [h["lr"] for h in hist] == [cosine_lr(3e-4, 0, 10), cosine_lr(3e-4, 1, 10), cosine_lr(1e-4, 2, 10),
                                       cosine_lr(1e-4, 3, 10)]


def test_flat_adam_refuses_another_length_before_it_writes():
    from deadtrees_amd.ops import FlatAdam
    p = torch.zeros(64, device=DEV)
    opt = FlatAdam(p)
    opt.set_trainable([(16, 64)])
    opt.m.fill_(1.0)
    opt.t_seg.fill_(3.0)
    sd = opt.state_dict()
    assert sd["_segments"] == [[0, 16], [16, 64]] and sd["_trainable"] == [False, True] and sd["t_seg"].tolist() == [3.0, 3.0]
    other = FlatAdam(torch.zeros(128, device=DEV))
    other.m.fill_(2.0)
    with pytest.raises(RuntimeError, match="elements"):
        other.load_state_dict(sd)
    assert other._segments is None and float(other.m.min()) == 2.0 and float(other.t_dev) == 0.0
    # and the matching length: in place, table derived
    same = FlatAdam(torch.zeros(64, device=DEV))
    ptrs = [t.data_ptr() for t in (same.m, same.v, same.t_dev, same.hyper, same.lr_dev)]
    same.load_state_dict(sd)
    assert ptrs == [t.data_ptr() for t in (same.m, same.v, same.t_dev, same.hyper, same.lr_dev)]
    assert same._segments == [(0, 16), (16, 64)] and same._trainable == [False, True]
    assert torch.equal(same.table, opt.table) and (same._table_rows, same._table_n, same._max_len) == \
        (opt._table_rows, opt._table_n, opt._max_len)
    assert torch.equal(same.m, opt.m) and torch.equal(same.t_seg, opt.t_seg) and same._lr_on_dev == opt._lr_on_dev


# -------------------------------------------------------------------------------------------- 6. inference readers
@pytest.mark.parametrize("decoder", ["unet", "resunet"])
def test_a_state_file_reads_like_any_checkpoint(decoder, tmp_path):
    from deadtrees_amd.network.segmodel import SemSegment
    path = tmp_path / "state.pt"
    tr = _state_file(path, decoder=decoder, epochs=2)
    m = tr.model
    loaded = SemSegment.load_from_checkpoint(str(path))
    want, got = m.smp_state_dict(), loaded.model.smp_state_dict()
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
    x = _loader()[0][0].to(DEV)
    m.eval()
    net = loaded.model.to(DEV).eval()
    with torch.no_grad():
        assert torch.equal(net(x), m(x))


# -------------------------------------------------------------------------------------------- beside: the epoch mean
def test_epoch_mean_of_replayed_steps_is_the_mean_of_their_losses():
    """a replayed step hands back the graph's static output: ``fit`` copies each value, so the history of a replayed run
    equals the eager run's (graph replay == eager); an epoch's record once was the LAST replayed step's loss, and a run
    resumed into two eager warm-up steps then disagreed with the uninterrupted one"""
    from deadtrees_amd.trainer import HipTrainer, fit
    hists = [fit(HipTrainer(_model(), graph=graph), _loader(), epochs=3, to_device=DEV) for graph in (False, True)]
    assert hists[0] == hists[1]
    assert len({h["train/total_loss"] for h in hists[1]}) == 3
