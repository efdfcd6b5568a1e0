"""``utils.graph_replay``: the warm-up / capture / copy-in / replay protocol and the two cache policies, on a pass of a
few torch ops (B = 2, 64 x 64).  The UNetHIP is there for its engine (``capture_workspaces``) only: no network runs."""
from unittest import mock

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE = (2, 3, 64, 64)


@pytest.fixture(scope="module")
def engine():
    from deadtrees_amd.network.unet import UNetHIP
    return UNetHIP(in_channels=3, classes=2).to(DEV).engine


def _fn(a, b):
    return a * 2 + (b if b is not None else 0)


def _pair(seed, with_b=True):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(SHAPE, generator=g).to(DEV)
    return a, (torch.randn(SHAPE, generator=g).to(DEV) if with_b else None)


def _replay(engine, warmup=2, **kw):
    from deadtrees_amd.utils.graph_replay import GraphReplay
    return GraphReplay(engine, _fn, warmup, **kw)


def _captured(engine, seed=100):
    """a GraphReplay past its two warm-up calls and its capture"""
    r = _replay(engine)
    for i in range(3):
        r(*_pair(seed + i))
    assert r.captured
    return r


def test_warm_up_then_capture_then_replays_equal_eager(engine):
    r = _replay(engine, warmup=2)
    assert not r.captured and r.graph is None and r.inputs is None and r.result is None
    for call in (1, 2):
        a, b = _pair(call)
        assert torch.equal(r(a, b), _fn(a, b))
        assert not r.captured, call
    a, b = _pair(3)
    out = r(a, b)                                      # call 3: capture, copy-in, replay
    assert r.captured and isinstance(r.graph, torch.cuda.CUDAGraph)
    assert out is r.result and torch.equal(out, _fn(a, b))
    graph = r.graph
    for call in (4, 5, 6):
        a, b = _pair(call)
        assert torch.equal(r(a, b), _fn(a, b)), call
        assert r.graph is graph and r.result is out    # one graph, one static output


def test_static_buffers_passed_back_are_not_copied(engine):
    real = torch.Tensor.copy_
    copies = []

    def counting(self, src, *args, **kwargs):
        copies.append((self.data_ptr(), src.data_ptr()))
        return real(self, src, *args, **kwargs)

    with mock.patch.object(torch.Tensor, "copy_", counting):
        r = _captured(engine)
        sa, sb = r.inputs
        ptrs = (sa.data_ptr(), sb.data_ptr())
        a, b = _pair(7)
        want = _fn(a, b)
        sa.copy_(a)
        sb.copy_(b)
        del copies[:]
        assert torch.equal(r(sa, sb), want)            # both inputs are the static buffers: no copy
        assert copies == []
        a2, b2 = _pair(8)
        assert torch.equal(r(sa, b2), _fn(a, b2))      # one is not: one copy, into its static buffer
        assert copies == [(sb.data_ptr(), b2.data_ptr())]
        del copies[:]
        assert torch.equal(r(a2, b2), _fn(a2, b2))
        assert copies == [(sa.data_ptr(), a2.data_ptr()), (sb.data_ptr(), b2.data_ptr())]
        assert r.inputs[0] is sa and r.inputs[1] is sb and (sa.data_ptr(), sb.data_ptr()) == ptrs
    assert torch.Tensor.copy_ is real


def test_none_input_stays_none_and_is_skipped(engine):
    r = _replay(engine, warmup=2)
    for i in range(4):
        a, _ = _pair(20 + i, with_b=False)
        assert torch.equal(r(a, None), _fn(a, None)), i
    assert r.captured and r.inputs[0] is not None and r.inputs[1] is None


def test_capture_workspaces_are_held_and_the_eager_ones_come_back(engine):
    eager_ws = engine._ws
    seen = []

    def fn(a, b):
        if torch.cuda.is_current_stream_capturing():
            seen.append(engine._ws)
            engine._buf("replay_probe", 16, device=a.device)      # a workspace allocated by the captured pass
        return _fn(a, b)

    from deadtrees_amd.utils.graph_replay import GraphReplay
    r = GraphReplay(engine, fn, 2)
    for i in range(4):
        a, b = _pair(30 + i)
        assert torch.equal(r(a, b), _fn(a, b))
    assert len(seen) == 1 and seen[0] is not eager_ws  # captured once, on a workspace dict of its own
    assert r.workspaces is seen[0] and "replay_probe" in r.workspaces
    assert engine._ws is eager_ws and "replay_probe" not in eager_ws


def test_keep_prefix_is_visible_inside_the_capture(engine):
    engine._ws["bf16_w_probe"] = torch.zeros(4, device=DEV)
    engine._ws["other_probe"] = torch.zeros(4, device=DEV)
    seen = []

    def fn(a, b):
        if torch.cuda.is_current_stream_capturing():
            seen.append(dict(engine._ws))
        return _fn(a, b)

    from deadtrees_amd.utils.graph_replay import GraphReplay
    try:
        r = GraphReplay(engine, fn, 1, keep=("bf16_w",))
        for i in range(2):
            r(*_pair(40 + i))
        assert r.captured and len(seen) == 1
        assert seen[0]["bf16_w_probe"] is engine._ws["bf16_w_probe"] and "other_probe" not in seen[0]
        assert "bf16_w_probe" in r.workspaces and "other_probe" not in r.workspaces
    finally:
        del engine._ws["bf16_w_probe"], engine._ws["other_probe"]


def test_separate_capture_callable_is_what_replays(engine):
    r = _replay(engine, warmup=1, capture_fn=lambda a, b: _fn(a, b) + 1)
    a, b = _pair(50)
    assert torch.equal(r(a, b), _fn(a, b))             # warm-up runs fn
    a, b = _pair(51)
    assert torch.equal(r(a, b), _fn(a, b) + 1)         # the graph holds capture_fn


def test_single_slot_cache_discards_and_warms_up_again(engine):
    from deadtrees_amd.utils.graph_replay import ReplayCache
    cache = ReplayCache(keep_all=False)
    made = []

    def make():
        made.append(_replay(engine, warmup=2))
        return made[-1]

    def call(key, seed):
        a, b = _pair(seed)
        r = cache.get(key, make)
        assert torch.equal(r(a, b), _fn(a, b))
        return r

    first = [call("k1", 60 + i) for i in range(3)]
    assert first[0] is first[1] is first[2] and first[0].captured and len(made) == 1
    second = call("k2", 63)
    assert second is not first[0] and not second.captured
    assert cache.keys() == ("k2",) and cache.values() == (second,)      # the first object is gone from the cache
    back = call("k1", 64)                              # returning to the first key: a fresh object, warming up again
    assert back is not first[0] and not back.captured and cache.values() == (back,) and len(made) == 3
    call("k1", 65)
    assert not back.captured
    assert call("k1", 66) is back and back.captured


def test_keep_all_cache_keeps_every_key(engine):
    from deadtrees_amd.utils.graph_replay import ReplayCache
    cache = ReplayCache(keep_all=True)
    made = []

    def make():
        made.append(_replay(engine, warmup=2))
        return made[-1]

    for key in ("k1", "k2"):
        for i in range(3):
            a, b = _pair(70 + i)
            assert torch.equal(cache.get(key, make)(a, b), _fn(a, b))
    assert len(cache) == 2 and len(made) == 2 and all(r.captured for r in cache.values())
    first, graph = cache.get("k1", make), made[0].graph
    assert first is made[0]
    a, b = _pair(80)
    assert torch.equal(first(a, b), _fn(a, b))         # back on the first key: a replay, no warm-up, no new object
    assert first.graph is graph and len(made) == 2
    cache.clear()
    assert len(cache) == 0
