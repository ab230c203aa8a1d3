"""Checkpoint I/O compatible with the reference's files:

* the legacy trainer writes ``torch.save(model.state_dict())`` to ``.../model.pth``
  (movenet/trainer.py:455-467), with a ``module.`` prefix when trained under DDP
  (:256-260);
* the Lightning trainer's checkpoints hold ``{"state_dict": {"model.<key>": ...}}``
  (movenet/pytorch_lightning_trainer.py:31 names the attribute ``model``).

Files are read with ``torch.load(..., weights_only=True)`` only: nothing in them is
executed.

The trainer's own checkpoints (``training_checkpoint`` / ``write_checkpoint``) add what a run needs to go on
where it stopped -- ``optimizer_states``, ``lr_schedulers``, ``hyper_parameters`` and ``resume`` -- to those keys;
``check_resumable`` is what ``Trainer.fit(ckpt_path=...)`` refuses a file by, before it touches the device.
"""
from __future__ import annotations

import os
from collections import OrderedDict
from dataclasses import asdict
from pathlib import Path
from typing import Dict, Optional

import torch

_PREFIXES = ("model.", "module.")

# what hyper_parameters records of the model's shape: the fields of config.ModelConfig, and what synthesize / evaluate
# build without a record and without the flag
MODEL_FIELDS = ("layer_size", "stack_size", "input_channels", "residual_channels", "skip_channels")
CLI_MODEL_DEFAULTS = {"input_channels": 256, "residual_channels": 64, "skip_channels": 64, "layer_size": 10,
                      "stack_size": 3}
# hyper_parameters a resumed run must share with the run that wrote the file (check_resumable), in the order checked
RESUME_FIELDS = MODEL_FIELDS + ("optimizer", "scheduler", "precision", "accumulation_steps", "batch_size",
                                "world_size")
HYPER_FIELDS = MODEL_FIELDS + ("precision", "bf16_video", "loss_rule", "optimizer", "scheduler", "accumulation_steps",
                               "batch_size", "world_size", "dataset")
RESUME_KEYS = ("epoch", "batches_done", "global_dropout_generator", "torch_rng", "history_len")


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
    ``audio_rate``), ``local_window`` where the run had ``--mel_window K > 0`` and ``f0`` where it had ``--mel_f0 1`` --
    or None for a file without one."""
    return _local_record(_read(path))


def local_window_of(rec) -> int:
    """The ``local_window`` of a ``"local_conditioning"`` record: the key is written only by a run with ``--mel_window
    K > 0``, so a record without it (every file written before the flag existed, and every K = 0 run) reads as 0."""
    return int(rec.get("local_window", 0)) if isinstance(rec, dict) else 0


def f0_record_of(rec):
    """The ``"f0"`` entry of a ``"local_conditioning"`` record -- ``{"f_min", "f_max", "f_ref"}``, the pitch search range
    in Hz and the frequency the log-F0 channel is 0 at -- or None: the key is written only by a run with ``--mel_f0 1``,
    so a record without it (every file written before the flag existed, and every ``--mel_f0 0`` run) reads as off."""
    f0 = rec.get("f0") if isinstance(rec, dict) else None
    return {k: float(f0[k]) for k in ("f_min", "f_max", "f_ref")} if isinstance(f0, dict) else None


def local_channels_of(rec) -> int:
    """The input channels of the ``local_conv`` a ``"local_conditioning"`` record describes: its ``local_channels`` mel
    bins, and the two F0 channels behind them where it has an ``"f0"`` entry."""
    return int(rec["local_channels"]) + (2 if f0_record_of(rec) else 0)


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
        model.set_local_conditioning(local_channels_of(rec), int(rec["local_hop"]), local_window_of(rec))
        model.local_conditioning = rec
    return model.load_state_dict(_state_dict_of(obj, path, ema), strict=strict)


# ---- the trainer's checkpoints: one writer, one reader --------------------------------------------------
def hyper_parameters(config, dataset: str, precision=32, bf16_video: bool = False, accumulation_steps: int = 1,
                     world_size: int = 1) -> dict:
    """The ``"hyper_parameters"`` record of a run: plain ints, floats, strings and bools only (the file stays loadable
    under ``weights_only=True``).  The five ``ModelConfig`` fields, what decides the run's arithmetic and its step
    count, and the dataset string.  ``precision`` is 32 or ``"bf16"``; a run without a scheduler records ``""``."""
    out = {k: int(v) for k, v in asdict(config.model_config).items()}
    out.update(precision=32 if precision in (32, "32") else str(precision), bf16_video=bool(bf16_video),
               loss_rule=str(getattr(config, "loss_rule", "reference")), optimizer=str(config.optimizer),
               scheduler="" if config.scheduler is None else str(config.scheduler),
               accumulation_steps=int(accumulation_steps), batch_size=int(config.batch_size),
               world_size=int(world_size), dataset=str(dataset))
    return out


def _on_cpu(obj, memo: dict):
    """``obj`` with every tensor replaced by a detached CPU copy -- one copy per tensor object, however often it occurs
    (``memo``: id -> copy) -- containers rebuilt, and entries that are code (a scheduler's scale function) left out."""
    if torch.is_tensor(obj):
        if id(obj) not in memo:
            memo[id(obj)] = obj.detach().cpu()
        return memo[id(obj)]
    if isinstance(obj, dict):
        return {k: _on_cpu(v, memo) for k, v in obj.items() if not callable(v)}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_on_cpu(v, memo) for v in obj if not callable(v))
    return obj


def training_checkpoint(module, optimizer, scheduler, *, epoch: int, global_step: int, next_epoch: int,
                        batches_done: int, hyper: dict, history_len: int) -> dict:
    """What the trainer writes: every key it wrote before, with the meaning it had --

    * ``epoch`` (the epoch the file was written in), ``global_step``, ``state_dict`` (Lightning's ``model.`` prefix),
      and where the run has them ``global_classes``, ``ema_state_dict`` / ``ema_decay`` / ``ema_updates``,
      ``local_conditioning``, ``preemphasis``;

    and what resuming needs --

    * ``optimizer_states``: ``[optimizer.state_dict()]`` on the CPU (``FlatAdamW``: the ``"flat"`` entry -- ``steps``,
      ``exp_avg``, ``exp_avg_sq``, with the average on ``ema`` and ``ema_updates`` -- plus ``param_groups``);
    * ``lr_schedulers``: ``[scheduler.state_dict()]``, ``[]`` without a scheduler;
    * ``hyper_parameters``: ``hyper`` (``hyper_parameters()``);
    * ``resume``: ``epoch``, the epoch the resumed run trains first, and ``batches_done``, how many of THAT epoch's
      batches are already consumed -- in an end-of-epoch file ``epoch`` is the NEXT epoch and ``batches_done`` is 0, in a
      mid-epoch ``last.ckpt`` it is the running epoch; ``global_dropout_generator`` and ``torch_rng``, the ``get_state()``
      byte tensors of the model's label-dropout generator and of torch's CPU generator; ``history_len``, the records
      the run has logged so far (= ``global_step``).

    With ``FlatAdamW`` each flat buffer crosses to the host ONCE: the per-name entries of ``state_dict`` and
    ``ema_state_dict`` are views of those copies (``torch.save`` stores a shared storage once)."""
    model = module.model
    named = dict(model.named_parameters())
    memo: dict = {}
    flat_views, ema_views = {}, {}
    if hasattr(optimizer, "flat"):
        averaging = getattr(optimizer, "ema_decay", 0.0) > 0
        flat = optimizer.flat.detach().cpu()
        ema = _on_cpu(optimizer.ema, memo) if averaging else None
        for p, o in zip(optimizer._params, optimizer._offsets):
            flat_views[id(p)] = flat[o:o + p.numel()].view(p.shape)
            if averaging:
                ema_views[id(p)] = ema[o:o + p.numel()].view(p.shape)
    else:
        averaging = False
    state, averaged = {}, {}
    for k, v in model.state_dict().items():
        pid = id(named[k]) if k in named else None
        state[f"model.{k}"] = flat_views[pid] if pid in flat_views else v.detach().cpu()
        if averaging:  # (optimizer.ema_state_dict's rule: buffers and parameters outside the optimizer as they are)
            averaged[f"model.{k}"] = ema_views[pid] if pid in ema_views else state[f"model.{k}"]
    names = list(getattr(module, "global_classes", []) or [])  # class i of global_embedding <-> names[i]
    gen = getattr(model, "global_dropout_generator", None)
    out = {"epoch": int(epoch), "global_step": int(global_step)}
    if names:
        out["global_classes"] = names
    if averaging:  # (absent without --ema_decay)
        out.update(ema_state_dict=averaged, ema_decay=optimizer.ema_decay, ema_updates=optimizer.ema_updates)
    if getattr(module, "use_mel", False):  # (--use_mel: what load_into rebuilds local_conv from; absent otherwise)
        out["local_conditioning"] = dict(module.local_conditioning)
    out.update(preemphasis_record(model))  # (--preemphasis A > 0: what load_into sets model.preemphasis from)
    out["state_dict"] = state
    out["optimizer_states"] = [_on_cpu(optimizer.state_dict(), memo)]
    out["lr_schedulers"] = [] if scheduler is None else [_on_cpu(scheduler.state_dict(), memo)]
    out["hyper_parameters"] = dict(hyper)
    out["resume"] = {"epoch": int(next_epoch), "batches_done": int(batches_done),
                     "global_dropout_generator": (gen if gen is not None else torch.Generator().manual_seed(0)).get_state(),
                     "torch_rng": torch.get_rng_state(), "history_len": int(history_len)}
    return out


def write_checkpoint(obj, path) -> None:
    """``torch.save`` into a temporary file beside ``path``, then ``os.replace``: ``path`` is the previous file or the
    new one, never part of one (a save that fails, or a run killed inside it, leaves the previous file as it was)."""
    path = Path(path)
    tmp = path.with_name(f".{path.name}.{os.getpid()}.tmp")
    try:
        torch.save(obj, tmp)
        os.replace(tmp, path)
    finally:
        if tmp.exists():
            tmp.unlink()


def read_checkpoint(path) -> dict:
    """The file, on the CPU, under ``weights_only=True``."""
    return _read(path)


def hyper_parameters_of(obj) -> dict:
    """The ``"hyper_parameters"`` record of a loaded checkpoint, or ``{}`` for a file without one."""
    rec = obj.get("hyper_parameters") if isinstance(obj, dict) else None
    return dict(rec) if isinstance(rec, dict) else {}


def global_classes_of(obj) -> list:
    """The ``"global_classes"`` names of a loaded checkpoint (class i of ``global_embedding`` <-> names[i]), ``[]`` for a
    file without them."""
    return list(obj.get("global_classes") or []) if isinstance(obj, dict) else []


def resolve_resume(value, output_path) -> Optional[Path]:
    """``--resume_from``: None or ``""`` -> None (a fresh run); ``"auto"`` -> ``<output_path>/checkpoints/last.ckpt`` if
    that file exists, else None; anything else is the path itself (FileNotFoundError if there is no such file)."""
    if value is None or str(value) == "":
        return None
    if str(value) == "auto":
        last = Path(output_path) / "checkpoints" / "last.ckpt"
        return last if last.is_file() else None
    if not Path(value).is_file():
        raise FileNotFoundError(f"--resume_from {value}: no such file")
    return Path(value)


def check_resumable(obj, path, run: dict, max_epochs: int, averaging: bool, local_window: int = 0, f0=None) -> None:
    """ValueError -- naming the file and the field -- for a checkpoint that ``Trainer.fit(ckpt_path=path)`` must not
    continue: one without ``optimizer_states`` (a file of weights: ``--pretrained_model_path`` takes those), one whose
    ``hyper_parameters`` disagree with the run's (``run``, from ``hyper_parameters()``) in any of ``RESUME_FIELDS``, one
    whose ``local_conditioning`` record holds another ``local_window`` than the run's ``--mel_window`` (absent: 0) or
    another ``f0`` entry than the run's (``f0``: ``{"f_min", "f_max", ...}`` under ``--mel_f0 1``, else None), one
    whose ``resume["epoch"]`` is not below ``max_epochs``, and -- with the weights' average on in the run -- one whose
    optimizer state holds no ``ema`` (``FlatAdamW.load_state_dict`` would start the average over without a word)."""
    if not isinstance(obj, dict) or not obj.get("optimizer_states"):
        raise ValueError(f"{path}: no 'optimizer_states' -- a checkpoint written before runs could be resumed, or a "
                         "file of weights only; start a new run from its weights with --pretrained_model_path")
    saved, resume = obj.get("hyper_parameters"), obj.get("resume")
    if not isinstance(saved, dict) or not isinstance(resume, dict):
        raise ValueError(f"{path}: no '{'resume' if isinstance(saved, dict) else 'hyper_parameters'}' record: not a "
                         "checkpoint a run can be resumed from")
    for field in RESUME_FIELDS:
        if saved.get(field) != run[field]:
            raise ValueError(f"{path}: hyper_parameters[{field!r}] is {saved.get(field)!r}, but this run has "
                             f"{run[field]!r}: a resumed run continues the run that wrote the file")
    saved_window = local_window_of(_local_record(obj))
    if saved_window != int(local_window):
        raise ValueError(f"{path}: local_conditioning['local_window'] is {saved_window}, but this run has "
                         f"{int(local_window)} (--mel_window): a resumed run continues the run that wrote the file")
    saved_f0 = f0_record_of(_local_record(obj))
    if (saved_f0 is None) != (f0 is None):
        raise ValueError(f"{path}: local_conditioning['f0'] is {'absent' if saved_f0 is None else 'present'}, but this "
                         f"run has --mel_f0 {int(f0 is not None)}: a resumed run continues the run that wrote the file")
    for key, flag in (("f_min", "--f0_min"), ("f_max", "--f0_max")):
        if saved_f0 is not None and saved_f0[key] != float(f0[key]):
            raise ValueError(f"{path}: local_conditioning['f0'][{key!r}] is {saved_f0[key]}, but this run has "
                             f"{float(f0[key])} ({flag}): a resumed run continues the run that wrote the file")
    if int(resume["epoch"]) >= int(max_epochs):
        raise ValueError(f"{path}: resume['epoch'] is {int(resume['epoch'])}, but this run ends after max_epochs = "
                         f"{int(max_epochs)}: nothing is left to train")
    if averaging:
        flat = obj["optimizer_states"][0].get("state", {}).get("flat")
        if not isinstance(flat, dict) or flat.get("ema") is None:
            raise ValueError(f"{path}: optimizer_states[0]['state']['flat'] holds no 'ema', but this run keeps an "
                             "average of the weights (--ema_decay): a resumed run must not restart its average")
