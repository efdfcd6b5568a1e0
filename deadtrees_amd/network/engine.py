"""``UNetEngine``: executes the layer list of ``UNetSpec`` on the C ABI — ONE object (one ``_ws``, one ``saved``, one
``launches`` / ``recal_launches`` / ``trace`` / ``profile``) assembled from the shared core, the two schedules and the
reverse schedule both of them run (``engine_backward``)."""
from __future__ import annotations

from .engine_backward import BackwardSchedule
from .engine_bf16 import Bf16Schedule
from .engine_core import EngineCore
from .engine_fp32 import Fp32Schedule


class UNetEngine(Fp32Schedule, Bf16Schedule, BackwardSchedule, EngineCore):
    """Executes the layer list of ``UNetSpec`` on the C ABI.  Holds no parameters itself."""
