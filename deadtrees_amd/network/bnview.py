"""The one owner of the two per-channel BatchNorm layouts.

``bnws``     per-forward workspace  ``[mean | invstd | scale | shift] x n_bn_channels``: row k of the convolution c is
             ``bnws[k * n_bn_channels + c.bn_off : ... + c.cout]``
``bn_state`` running statistics     ``[running_mean, running_var]`` per convolution, at ``2 * c.bn_off``

Pure slicing: works on device tensors (the engine) and on CPU copies (the state-dict converters, the host tests).
"""
from __future__ import annotations

from .. import _lib
from .spec import ConvSpec, UNetSpec


class BnView:
    __slots__ = ("nb", "ws", "state")

    def __init__(self, spec: UNetSpec, ws=None, state=None):
        self.nb = spec.n_bn_channels
        self.ws = ws            # float[4 * n_bn_channels] or None (state-only view)
        self.state = state      # float[2 * n_bn_channels] or None (workspace-only view: the backward passes)

    @staticmethod
    def ws_floats(spec: UNetSpec) -> int:
        return 4 * spec.n_bn_channels

    @staticmethod
    def state_floats(spec: UNetSpec) -> int:
        return 2 * spec.n_bn_channels

    def _row(self, k: int, c: ConvSpec):
        lo = k * self.nb + c.bn_off
        return self.ws[lo:lo + c.cout]

    def mean(self, c: ConvSpec):
        return self._row(0, c)

    def invstd(self, c: ConvSpec):
        return self._row(1, c)

    def scale(self, c: ConvSpec):
        return self._row(2, c)

    def shift(self, c: ConvSpec):
        return self._row(3, c)

    def ss(self, c: ConvSpec):
        """(scale, shift): what a consumer needs to apply conv c's BatchNorm (+ ReLU) to its raw output"""
        return self._row(2, c), self._row(3, c)

    def running_mean(self, c: ConvSpec):
        return self.state[2 * c.bn_off:2 * c.bn_off + c.cout]

    def running_var(self, c: ConvSpec):
        return self.state[2 * c.bn_off + c.cout:2 * c.bn_off + 2 * c.cout]

    def fuse(self, c: ConvSpec, y, act=None) -> "_lib.BnBwdFuse":
        """BatchNorm-backward reduction of conv c (raw output y) fused into the kernel that writes its output gradient.
        act None: the activation is virtual, its ReLU mask comes from y * scale + shift; else the stored block output."""
        asc, ash = self.ss(c) if act is None else (None, None)
        p = _lib.ptr
        return _lib.BnBwdFuse(p(y), p(self.mean(c)), p(self.invstd(c)), p(asc), p(ash), p(act))
