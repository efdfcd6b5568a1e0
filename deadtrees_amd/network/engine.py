"""``UNetEngine``: executes the layer list of ``UNetSpec`` on the C ABI — ONE object (one ``_ws``, one ``saved``, one
``launches`` / ``recal_launches`` / ``trace`` / ``profile``) assembled from the shared core, the units of
the two precisions, and the forward and reverse schedules both of them run (``engine_forward``, ``engine_backward``)."""
from __future__ import annotations

from .engine_backward import BackwardSchedule
from .engine_bf16 import Bf16Schedule
from .engine_core import EngineCore
from .engine_forward import ForwardSchedule
from .engine_fp32 import Fp32Schedule


class UNetEngine(Fp32Schedule, Bf16Schedule, ForwardSchedule, BackwardSchedule, EngineCore):
    """Executes the layer list of ``UNetSpec`` on the C ABI.  Holds no parameters itself."""
