"""Checkpoint I/O compatible with the reference's files:

* the legacy trainer writes ``torch.save(model.state_dict())`` to ``.../model.pth``
  (movenet/trainer.py:455-467), with a ``module.`` prefix when trained under DDP
  (:256-260);
* the Lightning trainer's checkpoints hold ``{"state_dict": {"model.<key>": ...}}``
  (movenet/pytorch_lightning_trainer.py:31 names the attribute ``model``).

Files are read with ``torch.load(..., weights_only=True)`` only: nothing in them is
executed.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict

import torch

_PREFIXES = ("model.", "module.")


def strip_prefixes(sd: Dict[str, torch.Tensor]) -> "OrderedDict[str, torch.Tensor]":
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for k, v in sd.items():
        changed = True
        while changed:
            changed = False
            for p in _PREFIXES:
                if k.startswith(p):
                    k, changed = k[len(p):], True
        out[k] = v
    return out


def _read(path):
    return torch.load(path, map_location="cpu", weights_only=True)


def load_state_dict_file(path, ema: bool = False) -> "OrderedDict[str, torch.Tensor]":
    """The weights in ``path``; with ``ema`` the averaged weights a run with ``--ema_decay`` saves beside them
    (``"ema_state_dict"``, same prefixes) -- ValueError for a file that holds none."""
    return _state_dict_of(_read(path), path, ema)


def _state_dict_of(obj, path, ema: bool) -> "OrderedDict[str, torch.Tensor]":
    if ema:
        if not (isinstance(obj, dict) and isinstance(obj.get("ema_state_dict"), dict)):
            raise ValueError(f"{path}: no 'ema_state_dict' (not a checkpoint of a run with --ema_decay > 0)")
        obj = obj["ema_state_dict"]
    elif isinstance(obj, dict) and "state_dict" in obj and isinstance(obj["state_dict"], dict):
        obj = obj["state_dict"]
    if not isinstance(obj, dict) or not all(torch.is_tensor(v) for v in obj.values()):
        raise ValueError(f"{path}: neither a state_dict nor a Lightning checkpoint")
    return strip_prefixes(obj)


def _local_record(obj):
    rec = obj.get("local_conditioning") if isinstance(obj, dict) else None
    return dict(rec) if isinstance(rec, dict) else None


def local_conditioning_of(path):
    """The ``"local_conditioning"`` record of a checkpoint trained with ``--use_mel 1`` -- ``local_channels``,
    ``local_hop`` and the mel settings its features were computed with (``mel_fft``, ``mel_fmin``, ``mel_fmax``,
    ``audio_rate``) -- or None for a file without one."""
    return _local_record(_read(path))


def _preemphasis_record(obj) -> float:
    v = obj.get("preemphasis", 0.0) if isinstance(obj, dict) else 0.0
    return float(v) if isinstance(v, (int, float)) and not isinstance(v, bool) else 0.0


def preemphasis_record(model) -> dict:
    """What a checkpoint of ``model`` carries beside its weights for ``--preemphasis``: ``{"preemphasis": a}`` for a
    model whose ``preemphasis`` is above 0, nothing otherwise (a run without the flag writes the file it wrote before)."""
    a = float(getattr(model, "preemphasis", 0.0))
    return {"preemphasis": a} if a > 0.0 else {}


def preemphasis_of(path) -> float:
    """The ``"preemphasis"`` record of a checkpoint trained with ``--preemphasis A`` -- the coefficient its training
    audio was pre-emphasised with -- or 0.0 for a file without one (the record is written only when A > 0)."""
    return _preemphasis_record(_read(path))


def load_into(model: torch.nn.Module, path, strict: bool = True, ema: bool = False):
    """model.load_state_dict from any of the reference's checkpoint flavours (``ema``: the averaged weights).  A
    checkpoint of a run with ``--use_mel 1`` carries its local-conditioning record: a model without a matching
    ``local_conv`` is given one first (``WaveNet.set_local_conditioning``, on the device of its other parameters), and
    the record is left in ``model.local_conditioning`` for whoever computes the features.  A checkpoint of a run with
    ``--preemphasis A`` sets ``model.preemphasis`` (a model that has the attribute; a file without the record leaves
    it as it is)."""
    obj = _read(path)  # (read once: the record and the weights come from the same object)
    if _preemphasis_record(obj) > 0.0 and hasattr(type(model), "preemphasis"):
        model.preemphasis = _preemphasis_record(obj)
    rec = _local_record(obj)
    if rec is not None and hasattr(model, "set_local_conditioning"):
        model.set_local_conditioning(int(rec["local_channels"]), int(rec["local_hop"]))
        model.local_conditioning = rec
    return model.load_state_dict(_state_dict_of(obj, path, ema), strict=strict)
