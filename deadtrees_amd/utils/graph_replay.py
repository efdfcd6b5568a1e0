"""HIP-graph capture and replay of one pass: the only place that builds a ``torch.cuda.CUDAGraph``, captures under
``torch.cuda.graph`` or enters ``engine.capture_workspaces``.

The protocol, once: run the pass eagerly ``warmup`` times (lazy initialisation — workspaces, device tables, autograd —
must never be captured), clone the inputs into static buffers, capture the pass on those buffers with the engine's
workspaces redirected into the graph's pool, then for every later call copy the new inputs in and replay.
"""
from __future__ import annotations

import gc
from typing import Callable, Optional, Sequence

import torch


class GraphReplay:
    """one pass ``fn(*inputs)`` (tensors, or None for an absent input) behind a warm-up counter and one captured graph.

    engine: owns ``capture_workspaces``; ``keep``: the eager workspace name prefixes the capture keeps (weight images
    packed eagerly).  ``capture_fn``: what is recorded instead of ``fn`` when the captured pass differs from the eager one
    (the training step skips its host bookkeeping); host work around the capture stays with the caller.  The static
    inputs, the workspace dict of the capture and the captured return value live exactly as long as this object; the
    result is the graph's static output: consume or copy it before the next call."""

    def __init__(self, engine, fn: Callable, warmup: int, keep: Sequence[str] = (), capture_fn: Optional[Callable] = None):
        self._engine, self._fn, self._capture_fn, self._keep = engine, fn, capture_fn or fn, tuple(keep)
        self._warm_left = int(warmup)
        self._graph = self._inputs = self._ws = self._result = None

    captured = property(lambda self: self._graph is not None, doc="the graph exists: calls replay it")
    graph = property(lambda self: self._graph, doc="the CUDAGraph (None before capture)")
    inputs = property(lambda self: self._inputs, doc="the static input buffers, None where the input was None")
    result = property(lambda self: self._result, doc="what the captured pass returned (the graph's static output)")
    workspaces = property(lambda self: self._ws, doc="the engine workspace dict of the capture (lives in the graph's pool)")

    def _capture(self, inputs):
        self._inputs = tuple(None if t is None else t.clone() for t in inputs)
        graph = torch.cuda.CUDAGraph()
        # workspaces of the captured pass live (and stay) in the graph's pool
        with self._engine.capture_workspaces(self._keep) as self._ws:
            torch.cuda.synchronize()
            # a cyclic collection that starts inside the capture tears down whatever garbage it finds — an earlier
            # trainer's graph and its pool, tensors with recorded streams — with calls a capturing stream does not allow,
            # and the process aborts.  torch.cuda.graph no longer collects on entry: collect here, and keep the collector
            # off until the capture has ended
            gc.collect()
            collecting = gc.isenabled()
            gc.disable()
            try:
                with torch.cuda.graph(graph):
                    self._result = self._capture_fn(*self._inputs)
            finally:
                if collecting:
                    gc.enable()
        self._graph = graph

    def __call__(self, *inputs):
        if self._graph is None:
            if self._warm_left > 0:
                self._warm_left -= 1
                return self._fn(*inputs)
            self._capture(inputs)
        # a caller that filled the static buffers itself hands them back: nothing to copy
        for static, t in zip(self._inputs, inputs):
            if t is not None and t is not static:
                static.copy_(t)
        self._graph.replay()
        return self._result


class ReplayCache:
    """key -> GraphReplay under one of two policies.  Single slot (``keep_all=False``): another key discards the held
    object — its graph pool is freed — and the new one warms up again.  ``keep_all=True``: one object per key, all kept."""

    def __init__(self, keep_all: bool):
        self.keep_all = bool(keep_all)
        self._slots = {}

    def get(self, key, make: Callable[[], GraphReplay]) -> GraphReplay:
        r = self._slots.get(key)
        if r is None:
            if not self.keep_all:
                self._slots.clear()
            r = self._slots[key] = make()
        return r

    def clear(self):
        self._slots.clear()

    def keys(self):
        return tuple(self._slots.keys())

    def values(self):
        return tuple(self._slots.values())

    def __len__(self):
        return len(self._slots)
