"""The full training state in one file: what ``fit(resume=...)`` needs to continue a run exactly.

One ``torch.save`` of a flat dict that ``torch.load(weights_only=True)`` reads — tensors, JSON strings and one integer;
no object is ever unpickled:

  format                       FORMAT (int)
  state_dict                   the smp-named tensors with the ``model.`` prefix   } exactly ``checkpoint_writer``'s payload:
  hyper_parameters_json        network / training configuration                  } every checkpoint reader reads the file
  trainer/flat_params          the RAW flat parameter buffer (alignment padding and the outer taps of a 1x1 head held as
                               a 3x3 kernel included: no smp key names them)
  trainer/bn_state, trainer/num_batches_tracked
  opt/m, opt/v, opt/t_dev, opt/hyper, opt/lr_dev [, opt/t_seg, opt/hyper_seg]
  average/avg                  (with HipTrainer(average=...))
  trainer_json                 description, module flags, the optimiser's host fields, the averager's mode / decay / count
  fit_json                     ``fit``'s state: epoch, history, schedule, SWA hand-over rate, selection state, ...
"""
from __future__ import annotations

import json
import os
from typing import Optional

import torch

FORMAT = 1
_OPT_TENSORS = ("m", "v", "t_dev", "hyper", "lr_dev", "t_seg", "hyper_seg")


def pack_training_state(trainer_state: dict, fit_state: dict, payload: Optional[dict] = None) -> dict:
    """``HipTrainer.state_dict()`` + ``fit``'s state (+ a checkpoint payload) -> the flat dict of the file"""
    opt, avg = trainer_state["opt"], trainer_state["averager"]
    out = {"format": FORMAT}
    if payload is not None:
        out["state_dict"] = payload["state_dict"]
        out["hyper_parameters_json"] = payload["hyper_parameters_json"]
    for name in ("flat_params", "bn_state", "num_batches_tracked"):
        out[f"trainer/{name}"] = trainer_state[name]
    for name in _OPT_TENSORS:
        if name in opt:
            out[f"opt/{name}"] = opt[name]
    if avg is not None:
        out["average/avg"] = avg["avg"]
    out["trainer_json"] = json.dumps({
        "description": trainer_state["description"], "flags": trainer_state["flags"],
        "opt": {k: v for k, v in opt.items() if k not in _OPT_TENSORS},
        "averager": None if avg is None else {k: v for k, v in avg.items() if k != "avg"}})
    out["fit_json"] = json.dumps(fit_state, default=float)      # (numpy scalars of a summary become floats)
    return out


def unpack_training_state(flat: dict) -> dict:
    """the file's flat dict -> {"format", "trainer": what ``HipTrainer.load_state_dict`` takes, "fit": ``fit``'s state}"""
    host = json.loads(flat["trainer_json"])
    opt = dict(host["opt"])
    for name in _OPT_TENSORS:
        if f"opt/{name}" in flat:
            opt[name] = flat[f"opt/{name}"]
    avg = host["averager"]
    if avg is not None:
        avg = dict(avg, avg=flat["average/avg"])
    trainer = {"description": host["description"], "flags": host["flags"], "opt": opt, "averager": avg}
    for name in ("flat_params", "bn_state", "num_batches_tracked"):
        trainer[name] = flat[f"trainer/{name}"]
    out = {"format": int(flat["format"]), "trainer": trainer, "fit": json.loads(flat["fit_json"])}
    for key in ("state_dict", "hyper_parameters_json"):
        if key in flat:
            out[key] = flat[key]
    return out


def save_training_state(path, trainer, fit_state: dict, pl_module=None, training_conf: Optional[dict] = None) -> bool:
    """Write the state file at ``path`` -> True when this process wrote it.

    trainer: a ``HipTrainer`` — its ``state_dict()`` and ``checkpoint_payload(trainer, pl_module, training_conf)`` go in, so
    ``SemSegment.load_from_checkpoint(path)`` and ``PyTorchInference(path)`` read the file like any checkpoint — or a
    trainer state dict taken earlier (the weights then go in only with a ``pl_module``).  Under data parallelism only rank
    0 writes.  The write is atomic: ``torch.save`` to ``path + ".tmp"`` in the same directory, then ``os.replace``; a
    failure leaves the previous file as it was and removes the temporary one."""
    path = os.fspath(path)
    if isinstance(trainer, dict):
        trainer_state, payload = trainer, None
        if pl_module is not None:
            from ..trainer import checkpoint_payload
            payload = checkpoint_payload(None, pl_module, training_conf)
    else:
        reducer = getattr(trainer, "reducer", None)
        if reducer is not None and trainer.world > 1 and reducer.dist.get_rank(reducer.group) != 0:
            return False
        from ..trainer import checkpoint_payload
        trainer_state = trainer.state_dict()
        payload = checkpoint_payload(trainer, pl_module, training_conf)
    flat = pack_training_state(trainer_state, fit_state, payload)
    tmp = path + ".tmp"
    try:
        torch.save(flat, tmp)
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise
    return True


def load_training_state(path, map_location="cpu") -> dict:
    """Read a state file with ``weights_only=True`` -> ``unpack_training_state``'s dict.  ValueError for a file of another
    ``format`` and for one without training state, such as the weights-only ``last.ckpt`` of ``checkpoint_writer``."""
    flat = torch.load(os.fspath(path), map_location=map_location, weights_only=True)
    no_state = ValueError(f"{path}: the file holds no training state (a weights-only checkpoint gives back a model, not a "
                          "run): resume needs a file written by fit(state=...)")
    if not isinstance(flat, dict) or "format" not in flat:
        raise no_state
    if isinstance(flat["format"], bool) or not isinstance(flat["format"], int) or flat["format"] != FORMAT:
        raise ValueError(f"{path}: unknown training state format {flat['format']!r}; this build reads format {FORMAT}")
    if "trainer_json" not in flat or "fit_json" not in flat:
        raise no_state
    return unpack_training_state(flat)
