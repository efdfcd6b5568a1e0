"""``PyTorchInference`` mirror (reference deadtrees/deployment/inference.py:30-62) on the HIP path.

Same contract: ``PyTorchInference(ckpt).run(tensor, device) -> int64 class map`` (``.squeeze()``-d), RGB slice
for a 3-channel model fed RGBN, ``ValueError`` for non-``.ckpt`` files, ``TypeError`` for non-tensors.
MI355X-first difference: forward + argmax are one fused pass (the head kernel emits the class map; the
logits never leave the GPU), and ``run_u8`` accepts raw uint8 tiles (normalisation fused on the device).
"""
from __future__ import annotations

from pathlib import Path
from typing import Union

import torch

from ..data.synthetic import MEAN, STD
from ..network.segmodel import SemSegment
from ..utils.graph_replay import GraphReplay, ReplayCache
from .. import ops


class Inference:
    """reference deployment/inference.py:14-27"""

    @property
    def in_channels(self):
        """band planes the network reads (infer_tile copies only these to the device); None while unknown"""
        return getattr(self, "_channels", None)

    def __init__(self, model_file: Union[str, Path]) -> None:
        self._model_file = model_file if isinstance(model_file, Path) else Path(model_file)

    @property
    def model_file(self) -> str:
        return self._model_file.name

    def run(self, input_tensor):  # pragma: no cover - abstract
        raise NotImplementedError


class ONNXInference(Inference):
    """reference deployment/inference.py:119-144.  The ONNX export of the reference (scripts/create_onnx.py) cannot
    carry the HIP kernels and onnxruntime is not part of this build: the class exists so that imports resolve."""

    def __init__(self, model_file) -> None:
        super().__init__(model_file)
        if self._model_file.suffix != ".onnx":
            raise ValueError(f"onnx file expected, but {self._model_file.suffix} received")
        raise NotImplementedError("ONNX inference is outside the MI355X hot path (SURVEY.md §8b); use PyTorchInference")


class PyTorchInference(Inference):
    def __init__(self, model_file: Union[str, Path]) -> None:
        super().__init__(model_file)
        if self._model_file.suffix != ".ckpt":
            raise ValueError(f"ckpt file expected, but {self._model_file.suffix} received")
        model = SemSegment.load_from_checkpoint(self._model_file)
        model.eval()
        self._channels = model.in_channels
        self._model = model.model

    @property
    def classes(self):
        """the model's class count (the K of the raster statistics), like the ensemble's"""
        return self._model.spec.classes

    def run(self, input_tensor, device: str = "cuda"):
        if not isinstance(input_tensor, torch.Tensor):
            raise TypeError("no pytorch tensor provided")
        self._model.to(device)
        if input_tensor.dim() == 3:
            input_tensor = input_tensor.unsqueeze(0)
        if self._channels == 3 and input_tensor.shape[1] == 4:
            input_tensor = input_tensor[:, 0:3, :, :]     # rgb model but rgbn data (inference.py:57-59)
        out = self._model.predict_classes(input_tensor.to(device).contiguous(), dtype="int64")
        return out.squeeze()

    def run_u8(self, tiles_u8_nhwc: torch.Tensor, device: str = "cuda") -> torch.Tensor:
        """uint8 [B,H,W,4] (what the tiler cuts) -> uint8 class map [B,H,W]; normalisation on the device
        (reference: per-tile albumentations Normalize on the CPU, scripts/inference.py:94-96)."""
        self._model.to(device)
        x = ops.normalize_u8(tiles_u8_nhwc.to(device), MEAN, STD, self._channels)   # NHWC f32: the kernels' layout
        return self._model.predict_classes(x, dtype="uint8", nhwc=True)

    def run_blocks(self, raster_chw_u8: torch.Tensor, d: int, first: int, count: int) -> torch.Tensor:
        """sub-tiles ``first`` .. ``first + count - 1`` of a band-major uint8 raster that already lives on the device ->
        uint8 class maps [count,d,d]: block split + zero padding + Normalize + channel selection are ONE gather
        (``dt_split_normalize_u8``) straight into the stem's NHWC input"""
        self._model.to(raster_chw_u8.device)
        x = ops.split_normalize_u8(raster_chw_u8, d, first, count, MEAN, STD, self._channels)
        return self._model.predict_classes(x, dtype="uint8", nhwc=True)

    def run_windows(self, raster_chw_u8: torch.Tensor, d: int, overlap: int, first: int, count: int,
                    want: str = "classes", precision: str = "fp32", views=None) -> torch.Tensor:
        """``run_blocks`` on the overlap-stitch grid (``tiler.window_grid``: origins ``d - overlap`` apart; overlap 0 is
        the block grid): windows ``first`` .. ``first + count - 1`` through ONE gather (``dt_window_normalize_u8``) and the
        forward -> ``want="classes"``: uint8 class maps [count,d,d] (fused argmax, for ``ops.stitch_classes``);
        ``want="logits"``: fp32 NCHW logits [count,K,d,d] (for ``ops.stitch_accumulate``).  ``views`` (T (flip, rot) pairs,
        ``tiler.tta_views``): every window goes through the network once per view (the same gather cuts the views) ->
        logits [count,T,K,d,d], still in view orientation (``ops.stitch_accumulate(views=...)`` maps them back); a class
        map cannot be averaged, so ``want="classes"`` with views is a ``ValueError``"""
        if want not in ("classes", "logits"):
            raise ValueError(f"want {want!r}: use 'classes' or 'logits'")
        if views is not None and want == "classes":
            raise ValueError("run_windows: views need want='logits' (class maps of several views cannot be averaged)")
        self._model.to(raster_chw_u8.device)
        x = ops.window_normalize_u8(raster_chw_u8, d, overlap, first, count, MEAN, STD, self._channels, views=views)
        if want == "classes":
            return self._model.predict_classes(x, dtype="uint8", precision=precision, nhwc=True)
        logits = self._model.predict_logits(x, precision=precision, nhwc=True)
        return logits if views is None else logits.reshape(count, len(views), *logits.shape[1:])

    @staticmethod
    def is_valid_raster(raster_chw_u8: torch.Tensor) -> bool:
        """scripts/inference.py:60-62 ``is_valid_tile`` on a raster in HBM: False when band 1 holds only 0 / 255"""
        return bool(int(ops.band_has_data(raster_chw_u8[0])) != 0)


class PyTorchEnsembleInference:
    """reference deployment/inference.py:65-116: an odd number of checkpoints, per-pixel majority (torch.mode) of
    their class maps.  Here every model emits a uint8 map from the fused head kernel and one vote kernel
    (``dt_ensemble_vote``, ties -> smallest class like torch.mode) replaces stack + mode.

    ``vote`` says how ``tiler.infer_tile`` combines the members over a whole raster (``.run`` is always the reference's
    hard vote): ``"hard"`` (default) — the majority of the members' raster class maps; ``"soft"`` — the members'
    probabilities are added into one accumulator and the map is its argmax.  ``members`` are the ``PyTorchInference``
    objects the tiler runs window batches through."""

    def __init__(self, *model_files: Union[str, Path], vote: str = "hard"):
        self._models, self._members, self._channels, self._classes = [], [], None, None
        if vote not in ("hard", "soft"):
            raise ValueError(f"vote {vote!r}: use 'hard' or 'soft'")
        self.vote = vote
        if len(model_files) % 2 == 0:
            raise ValueError("PyTorchEnsembleInference requires an uneven number of models")
        for model_file in model_files:
            model_file = Path(model_file)
            if model_file.suffix != ".ckpt":
                raise ValueError(f"Ckpt file expected, but {model_file.suffix} received")
            member = PyTorchInference(model_file)
            channels, classes = member.in_channels, member._model.spec.classes
            if not self._channels:
                self._channels, self._classes = channels, classes
            if channels != self._channels or classes != self._classes:
                raise ValueError("Models are not compatible since they were trained for different channel configs")
            self._members.append(member)
            self._models.append(member._model)

    @property
    def members(self):
        """one ``PyTorchInference`` per checkpoint, in the order given"""
        return tuple(self._members)

    @property
    def in_channels(self):
        """band planes the members read (infer_tile copies only these to the device)"""
        return self._channels

    @property
    def classes(self):
        return self._classes

    def run(self, input_tensor, device: str = "cuda"):
        if not isinstance(input_tensor, torch.Tensor):
            raise TypeError("No PyTorch tensor provided")
        if input_tensor.dim() == 3:
            input_tensor = input_tensor.unsqueeze(0)
        if self._channels == 3 and input_tensor.shape[1] == 4:
            input_tensor = input_tensor[:, 0:3, :, :]     # rgb model but rgbn data
        x = input_tensor.to(device).contiguous()
        maps = torch.stack([m.to(device).predict_classes(x, dtype="uint8") for m in self._models], dim=0)
        out, _ = ops.ensemble_vote(maps, self._classes, dtype="int64")
        return out.squeeze()


class GraphedTilePredictor:
    """uint8 NHWC tiles -> uint8 class maps with the whole chain (normalise, U-Net forward, argmax) replayed as ONE
    HIP graph per batch shape (``utils.graph_replay``): ~120 Python launches per batch become one, which keeps the tile queue of
    scripts/inference.py:80-115 independent of host jitter (eight ranks sharing a node).  On an idle host the eager
    chain is already GPU-bound (bench.py --mode infer: same rate with and without the graph).  The returned tensor is the graph's static output: consume or copy it before the next
    call.  Weights are read from the engine's cached images, so a model whose parameters change must run one eager
    ``predict_classes`` (which repacks them) before further replays."""

    def __init__(self, model, in_channels: int = 3, precision: str = "fp32"):
        self.model, self.c, self.precision = model, in_channels, precision
        self.in_channels = in_channels
        self._replays = ReplayCache(keep_all=True)

    def _eager(self, tiles_u8):
        x = ops.normalize_u8(tiles_u8, MEAN, STD, self.c)
        return self.model.predict_classes(x, dtype="uint8", precision=self.precision, nhwc=True)

    def __call__(self, tiles_u8: torch.Tensor) -> torch.Tensor:
        # activations / scratch of the capture live in the graph's pool; the bf16 weight images packed eagerly stay
        r = self._replays.get((tuple(tiles_u8.shape), tiles_u8.device),
                              lambda: GraphReplay(self.model.engine, self._eager, warmup=1, keep=("bf16_w",)))
        if not r.captured:
            r(tiles_u8)                                # warm-up: lazy initialisation + weight images packed eagerly
        return r(tiles_u8)                             # (first call of a key: capture;) copy in, replay
