"""The poison harness (tests/poison.py) catches what it is for: host only, fake "ops" in Python on CPU tensors that
allocate through torch.empty.  A correct op passes the three-run comparison; each of five broken ones fails, with the
allocation site named."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poison  # noqa: E402
from poison import GuardError, PoisonError, check_guards, guarded, poisoned, run_three, same_bytes  # noqa: E402

HERE = os.path.join("tests", os.path.basename(__file__))


def _line(marker: str) -> str:
    """"tests/test_poison_host.py:<line>" of the one source line that carries ``# site: <marker>``"""
    with open(os.path.abspath(__file__)) as f:
        hits = [i + 1 for i, text in enumerate(f) if text.rstrip().endswith(f"# site: {marker}")]
    assert len(hits) == 1, (marker, hits)
    return f"{HERE}:{hits[0]}"


def _past(t, k):
    """element k of the storage behind t, counted from t[0] (k = -1: the element before, k = numel: the one past)"""
    return t.as_strided((1,), (1,), t.storage_offset() + k)


# ---- the fake ops: x fp32 [n] -> 2 * x
def op_correct(x):
    ws = torch.empty(4, dtype=torch.float32)
    ws[:] = 2.0
    out = torch.empty(x.numel(), dtype=torch.float32)
    idx = torch.empty(x.numel(), dtype=torch.int64)
    idx.copy_(torch.arange(x.numel()))
    out.copy_(x[idx] * ws[0])
    return out, idx


def op_unset_element(x):
    out = torch.empty(x.numel(), dtype=torch.float32)  # site: unset
    out[:-1] = 2.0 * x[:-1]
    if not poison._active:
        out[-1] = 2.0 * x[-1]          # what a recycled allocator block looks like: the previous, correct, answer
    return out


def op_stale_workspace(x):
    ws = torch.empty(4, dtype=torch.float32)  # site: stale
    if not poison._active:
        ws.zero_()
    return 2.0 * x + ws[0] * 0.0


def op_write_past(x):
    out = torch.empty(x.numel(), dtype=torch.float32)  # site: past
    out.copy_(2.0 * x)
    _past(out, out.numel()).fill_(7.0)
    return out


def op_write_before(x):
    out = torch.empty(x.numel(), dtype=torch.int32)  # site: before
    out.copy_((2.0 * x).int())
    _past(out, -1).fill_(1)
    return out


def op_read_past_input(x):
    out = torch.empty(x.numel(), dtype=torch.float32)
    out.copy_(2.0 * x)
    out[-1] += _past(x, x.numel())[0] * 0.0
    return out


def _x():
    return (torch.arange(1, 12, dtype=torch.float32) / 8,)


def test_correct_op_passes():
    flat = run_three(_x, op_correct)
    assert [p for p, _ in flat] == ["out[0]", "out[1]"]
    assert torch.equal(flat[0][1], 2.0 * _x()[0])


def test_unset_output_element_fails():
    with pytest.raises(PoisonError) as e:
        run_three(_x, op_unset_element)
    assert _line("unset") in str(e.value) and "flat index 10" in str(e.value), str(e.value)


def test_stale_workspace_read_fails():
    """the product with zero hides the sentinel and shows the NaN: this is why there are two poisons"""
    with pytest.raises(PoisonError) as e:
        run_three(_x, op_stale_workspace)
    assert _line("stale") in str(e.value) and "poisoned(nan, 0)" in str(e.value), str(e.value)
    with poisoned(poison.SENTINEL, 1):
        assert torch.equal(op_stale_workspace(*_x()), 2.0 * _x()[0])


def test_write_past_output_fails():
    # only under the harness: on plain memory the same store would land in the allocator's slack
    with pytest.raises(GuardError) as e:
        with poisoned(poison.NAN, 0):
            op_write_past(*_x())
    assert _line("past") in str(e.value) and "behind the buffer" in str(e.value), str(e.value)
    assert "the nearest 0 byte(s) away" in str(e.value), str(e.value)


def test_write_before_output_fails():
    """an integer store of 1 before an integer buffer: the guards hold 1 per 8-byte word in the run whose poison is 0 and
    zeros in the other, so the store shows in at least one of the two"""
    caught = []
    for fills in ((poison.NAN, 0), (poison.SENTINEL, 1)):
        try:
            with poisoned(*fills):
                op_write_before(*_x())
        except GuardError as e:
            caught.append(str(e))
    assert caught and all(_line("before") in m and "before the buffer" in m for m in caught), caught


def test_read_past_guarded_input_fails():
    x = guarded(_x()[0])
    try:
        out = op_read_past_input(x)
        assert bool(torch.isnan(out[-1])) and torch.equal(out[:-1], 2.0 * x[:-1])
    finally:
        poison.release_inputs()
    with pytest.raises(PoisonError, match="a read outside an input") as e:
        run_three(_x, op_read_past_input)  # site: read past
    assert _line("read past") in str(e.value) and "input[0] (11 x torch.float32)" in str(e.value), str(e.value)


def test_check_guards_callable_inside_the_block():
    with pytest.raises(GuardError):
        with poisoned(poison.NAN, 0):
            out = torch.empty(3)
            check_guards()
            _past(out, 3).fill_(0.0)
            check_guards()


def test_names_restored_after_exception():
    before = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty, torch.zeros, torch.full)
    had = "new_empty" in torch.Tensor.__dict__
    with pytest.raises(ZeroDivisionError):
        with poisoned(poison.NAN, 0):
            assert torch.empty is not before[0] and torch.Tensor.new_empty is not before[3]
            1 / 0
    after = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty, torch.zeros, torch.full)
    assert all(a is b for a, b in zip(before, after))
    assert ("new_empty" in torch.Tensor.__dict__) == had
    assert not poison._active
    assert torch.empty(2, 3).shape == (2, 3)


DTYPES = (torch.float32, torch.bfloat16, torch.float64, torch.int64, torch.int32, torch.int16, torch.uint8, torch.bool,
          torch.uint16)


@pytest.mark.parametrize("fills", [(poison.NAN, 0), (poison.SENTINEL, 1)], ids=["nan0", "sentinel1"])
def test_views_alignment_and_poison(fills):
    like = torch.zeros(3, 5, dtype=torch.int32)
    with poisoned(*fills, wide_u8=("_wide_workspace",)) as state:
        made = []
        for dt in DTYPES:
            made += [torch.empty((3, 5), dtype=dt), torch.empty(7, dtype=dt), torch.empty_like(like, dtype=dt),
                     like.new_empty((2, 3), dtype=dt), torch.empty_strided((3, 5), (5, 1), dtype=dt),
                     torch.empty(0, dtype=dt)]
        made.append(torch.empty_strided((3, 2), (1, 4), dtype=torch.float32))
        assert made[-1].stride() == (1, 4)
        for t in made[:-1]:
            assert t.is_contiguous() and (t.numel() == 0 or t.data_ptr() % 256 == 0), (t.dtype, t.shape)
        for t in made:
            if t.numel() == 0:
                continue
            if t.dtype.is_floating_point:
                flat = t.as_strided((t.numel(),), (1,)) if t is not made[-1] else t.reshape(-1)
                assert bool(torch.isnan(flat).all()) if fills[0] != fills[0] else bool((flat.double() > 9e29).all())
            elif t.dtype == torch.bool:
                assert bool((t == bool(fills[1])).all())
            elif t.dtype == torch.uint16:
                assert bool((t.view(torch.int16) == fills[1]).all())
            else:
                assert bool((t == fills[1]).all()), t.dtype          # the element value, never a byte pattern
        ws = _wide_workspace(43)
        assert ws.dtype == torch.uint8 and int(ws.max()) <= 1
        words = ws[:40].view(torch.int64)
        assert bool((words == fills[1]).all()) and int(ws[40:].to(torch.int64).sum()) <= fills[1]
        z, f = torch.zeros((2, 3), dtype=torch.int32), torch.full((5,), -1, dtype=torch.int64)
        assert int(z.abs().sum()) == 0 and bool((f == -1).all()) and torch.full((2,), 1.5).dtype == torch.float32
        assert len(state.records) == len(made) + 4
        assert torch.empty(2, 3).shape == (2, 3) and torch.empty([2, 3]).shape == (2, 3)


def _wide_workspace(n):
    return torch.empty(n, dtype=torch.uint8)


def test_zeros_and_full_are_guarded():
    with pytest.raises(GuardError):
        with poisoned(poison.NAN, 0):
            z = torch.zeros(5, dtype=torch.float32)
            _past(z, 5).fill_(0.0)
    with pytest.raises(GuardError):
        with poisoned(poison.SENTINEL, 1):
            f = torch.full((5,), -1, dtype=torch.int32)
            _past(f, -1).fill_(-1)


def test_same_bytes():
    nan = torch.tensor([float("nan"), 1.0])
    assert same_bytes(nan, nan.clone()) and not torch.equal(nan, nan.clone())
    assert not same_bytes(torch.tensor([0.0]), torch.tensor([-0.0])) and torch.equal(torch.tensor([0.0]), torch.tensor([-0.0]))
    assert not same_bytes(torch.zeros(2), torch.zeros(3)) and not same_bytes(torch.zeros(2), torch.zeros(2, dtype=torch.int32))
    assert same_bytes(torch.zeros(0), torch.zeros(0))


def test_guarded_copy():
    x = torch.arange(6, dtype=torch.float32).view(2, 3).t()                 # not contiguous
    g = guarded(x)
    i = guarded(torch.arange(5, dtype=torch.int64))
    try:
        assert g.is_contiguous() and torch.equal(g, x) and g.data_ptr() % 256 == 0
        assert bool(torch.isnan(_past(g, 6)).all()) and bool(torch.isnan(_past(g, -1)).all())
        assert int(_past(i, 5)) == 0 and int(_past(i, -1)) == 0
        check_guards()
        _past(i, 5).fill_(3)
        with pytest.raises(GuardError, match=HERE):
            check_guards()
    finally:
        poison.release_inputs()


def test_blocks_do_not_nest_and_bad_fills_are_refused():
    with poisoned(poison.NAN, 0):
        with pytest.raises(RuntimeError, match="nest"):
            with poisoned(poison.NAN, 0):
                pass
    with pytest.raises(ValueError):
        with poisoned(poison.NAN, 0xA5):
            pass
    assert not poison._active and torch.empty.__module__ != poison.__name__
