"""Host side of stochastic weight averaging: the SWALR closed form against torch's scheduler, and the argument checks
of ``fit(swa=...)``.  No GPU."""
import types

import pytest
import torch


@pytest.mark.parametrize("strategy", ["cos", "linear"])
@pytest.mark.parametrize("anneal_epochs", [1, 2, 5, 10])
@pytest.mark.parametrize("lr0,target", [(3e-4, 1e-4), (1e-3, 5e-2), (2.5e-5, 3e-4)])
def test_swa_lr_is_torch_swalr(strategy, anneal_epochs, lr0, target):
    """``swa_lr`` against ``torch.optim.swa_utils.SWALR`` stepped once per epoch on a dummy SGD optimiser, 25 epochs.
    Both are double arithmetic on the host (torch's is recursive, this one closed): equal to 1e-12 relative."""
    from torch.optim.swa_utils import SWALR
    from deadtrees_amd.trainer import swa_lr
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr0)
    sched = SWALR(opt, swa_lr=target, anneal_epochs=anneal_epochs, anneal_strategy=strategy)
    worst = 0.0
    for e in range(25):
        want = opt.param_groups[0]["lr"]
        got = swa_lr(e, lr0, target, anneal_epochs, strategy)
        worst = max(worst, abs(got - want) / abs(want))
        assert got == pytest.approx(want, rel=1e-12, abs=0.0), (e, got, want)
        opt.step()
        sched.step()
    print(f"swa_lr vs SWALR ({strategy}, {anneal_epochs}, {lr0}->{target}): worst relative difference {worst:.2e}")


def test_swa_lr_without_annealing_and_bad_arguments():
    from torch.optim.swa_utils import SWALR
    from deadtrees_amd.trainer import swa_lr
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1e-3)
    sched = SWALR(opt, swa_lr=2e-4, anneal_epochs=0)
    for e in range(3):      # anneal_epochs = 0: torch sets swa_lr at once
        assert swa_lr(e, 1e-3, 2e-4, 0) == pytest.approx(opt.param_groups[0]["lr"], rel=1e-12)
        opt.step()
        sched.step()
    with pytest.raises(ValueError):
        swa_lr(0, 1e-3, 2e-4, 10, "exp")
    with pytest.raises(ValueError):
        swa_lr(-1, 1e-3, 2e-4, 10)


class _NoBatches:
    """a loader that must not be touched: the checks come before the first step"""

    def __iter__(self):
        raise AssertionError("fit() started to train before it checked its arguments")


def _stub_trainer(mode):
    av = None if mode is None else types.SimpleNamespace(mode=mode)
    return types.SimpleNamespace(averager=av, opt=types.SimpleNamespace(lr=0.0), model=None)


@pytest.mark.parametrize("cfg", [
    dict(swa_start=5), dict(swa_start=7), dict(swa_start=-1), dict(swa_start=2, anneal_epochs=-3),
    dict(swa_start=2, swa_lr=-1e-3), dict(swa_start=2, anneal_strategy="exp"), dict(swa_start=1.5)])
def test_fit_rejects_bad_swa_arguments_before_the_first_step(cfg):
    from deadtrees_amd.trainer import SWAConfig, fit
    with pytest.raises(ValueError):
        fit(_stub_trainer("swa"), _NoBatches(), epochs=5, swa=SWAConfig(**cfg))


@pytest.mark.parametrize("mode", [None, "ema"])
def test_fit_swa_needs_an_swa_trainer(mode):
    from deadtrees_amd.trainer import SWAConfig, fit
    with pytest.raises(ValueError, match="average='swa'"):
        fit(_stub_trainer(mode), _NoBatches(), epochs=5, swa=SWAConfig(swa_start=2))
    with pytest.raises(ValueError):
        fit(_stub_trainer(mode), _NoBatches(), epochs=5, swa=True)
    with pytest.raises(ValueError):
        fit(_stub_trainer("swa"), _NoBatches(), epochs=5, swa="yes")


def test_swa_true_resolves_to_the_documented_defaults():
    from deadtrees_amd.trainer import SWAConfig, resolve_swa
    assert resolve_swa(None, 50, 3e-4) is None
    assert resolve_swa(True, 50, 3e-4) == SWAConfig(swa_start=40, swa_lr=3e-4, anneal_epochs=10, anneal_strategy="cos")
    assert resolve_swa(True, 7, 1e-3) == SWAConfig(swa_start=5, swa_lr=1e-3, anneal_epochs=10, anneal_strategy="cos")
    assert resolve_swa(SWAConfig(3, swa_lr=None, anneal_epochs=4, anneal_strategy="linear"), 9, 2e-4) == \
        SWAConfig(3, 2e-4, 4, "linear")


def test_average_mode_parsing():
    from deadtrees_amd.ops import parse_average
    assert parse_average("swa") == ("swa", 0.0)
    assert parse_average(("ema", 0.99)) == ("ema", 0.99)
    assert parse_average("ema") == ("ema", 0.999)       # torch's get_ema_multi_avg_fn default
    for bad in ("mean", ("ema", 1.5), ("ema", -0.1), ("swa", 0.5)):
        with pytest.raises(ValueError):
            parse_average(bad)
