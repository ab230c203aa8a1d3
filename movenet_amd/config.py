"""Model / training configuration and CLI flags of the trainer entry point.

Same dataclass fields, defaults and flag names as the reference
(/root/reference/movenet/config.py:11-94 dataclasses, :149-240 argparse), so a
command line written for ``movenet/pytorch_lightning_trainer.py`` parses here
unchanged.  ``dataclasses_json`` is not available offline; ``to_json`` /
``from_json`` are provided directly.  Kept quirk: the
``--gradient_clipping`` flag is parsed but never copied into the config.
"""
from __future__ import annotations

import argparse
import json
from dataclasses import asdict, dataclass, field, fields
from datetime import datetime
from pathlib import Path
from typing import List, Optional


@dataclass
class ModelConfig:
    layer_size: int = 2
    stack_size: int = 2
    input_channels: int = 256
    residual_channels: int = 16
    skip_channels: int = 16


@dataclass
class TrainingConfig:
    model_config: ModelConfig = field(default_factory=ModelConfig)

    batch_size: int = 3
    val_batch_size: int = 3
    checkpoint_every: int = 25
    optimizer: str = "AdamW"
    learning_rate: float = 0.0001
    momentum: float = 0.9
    accumulation_steps: int = 1
    num_workers: int = 0
    val_num_workers: int = 0
    pin_memory: bool = False
    weight_decay: float = 0.0
    n_epochs: int = 100
    n_steps_per_epoch: Optional[int] = None
    use_video: bool = True
    gradient_clipping: Optional[float] = 0.0
    batch_subsample_frac: Optional[float] = None
    val_batch_subsample_frac: Optional[float] = None

    generate_n_samples: Optional[int] = None
    generate_temperature: float = 1.0
    # what a sampled generate() step draws from (WaveNet.generate_sampling): "reference", the reference's
    # softmax(softmax(logits) / T), or "model", the model's own softmax(logits / T).  Not a field of the
    # reference's config: a JSON written without it loads with the default.
    generate_sampling: str = "reference"
    # truncation of a sampled step before the draw (WaveNet.generate_top_k / generate_top_p): the k likeliest classes
    # (0: off), then the smallest head of them that holds p of their mass (1.0: off).  Not reference fields either.
    generate_top_k: int = 0
    generate_top_p: float = 1.0
    # temperatures each logged clip is generated at, all in ONE generate() call (empty: off -- generate_temperature
    # alone, as before); the sample logger then writes one file per clip and temperature.  Not a reference field.
    generate_temperature_sweep: List[float] = field(default_factory=list)

    # what the train step minimises (WaveNet.loss_rule): "reference", the reference's cross_entropy applied to the
    # model's probabilities, or "model", cross_entropy of the logits (the negative log-likelihood of the distribution
    # --generate_sampling model draws from).  Not a reference field: a JSON written without it loads with the default.
    loss_rule: str = "reference"

    # global conditioning on the clip's class label (WaveNet(global_classes=...)): the sorted context folders
    # of the training set are the classes and every batch's context names go to forward() as global_features.  Not a
    # reference field: a JSON written without it loads with the default (off).
    use_global: bool = False
    # Trainer(precision="bf16") with use_video: opt in to the video context on bf16 operands (WaveNet.bf16_context; not a
    # reference field)
    bf16_video: bool = False
    # classifier-free guidance of a labelled model.  generate_guidance: the scale the sample logger
    # generates with (WaveNet.generate_guidance; 1.0: off, plain conditional generation).  global_dropout: with this
    # probability per sequence and TRAIN step the label's vector is replaced by zeros, so that the model also learns
    # the "no label" condition guidance needs (never in validation or sampling).  Not reference fields: a JSON written
    # without them loads with the defaults (off).
    generate_guidance: float = 1.0
    global_dropout: float = 0.0
    # raw uint8 frames in a WAV folder (WavFolderLoader): video_antialias is the resize rule of the GPU front
    # end (False: torchvision 0.13 - 0.16's resize of a tensor; True: the default of 0.17 on).  Not a reference field:
    # a JSON written without it loads with the default.
    video_antialias: bool = False

    # exponential moving average of the weights, kept by the fused optimizer step (FlatAdamW(ema_decay=...), DESIGN
    # 4.6): 0 is off; above 0, validation, the logged samples and the checkpoint's "ema_state_dict" come from the
    # averaged weights.  ema_warmup ramps the decay as min(ema_decay, (1 + t) / (10 + t)).  Not reference fields: a JSON
    # written without them loads with the defaults (off).
    ema_decay: float = 0.0
    ema_warmup: bool = True

    # sample logger: also score each logged batch (WaveNet.score, one call per batch) and write bits_per_sample -- of
    # the generated clip under the conditioning it was generated with -- and source_bits_per_sample -- of the clip it
    # was prompted from -- into the clip's index.jsonl rows.  Not a reference field: a JSON written without it loads
    # with the default (off: no row changes).
    score_samples: bool = False
    # ... and, with use_mel, track the pitch of each generated clip and of its source (WaveNet.pitch_distance, one call
    # per logged batch): f0_rmse_cents, vuv_error_rate and gross_pitch_error_rate in the rows.  Needs
    # score_samples and use_mel.  Not a reference field: a JSON written without it loads with the default (off).
    score_pitch: bool = False

    # clips of a WAV folder at their own length (WavFolderLoader): "resample" stretches every clip onto
    # the batch width (the reference's rule); "native" resamples every clip to audio_rate, pads the batch to that width
    # and leaves the padding out of the loss.  Not reference fields: a JSON written without them loads with the defaults.
    # "window" trains on random windows of long recordings: rows are `frames` consecutive samples of a
    # file's resample to audio_rate, normalised by the whole file's range (window_gain "file") or the window's own
    # ("window").
    clip_length: str = "resample"
    audio_rate: int = 16000
    window_gain: str = "file"

    # local conditioning on the clip's own log-mel frames (WaveNet(local_channels=mel_bins, local_hop=mel_hop), DESIGN
    # 4.5d): every batch's features are computed on the GPU from its class indices (ops.logmel: frames of mel_fft samples
    # mel_hop apart, an HTK filterbank of mel_bins triangles from mel_fmin to mel_fmax Hz at audio_rate; mel_fmax None:
    # audio_rate / 2) and go to forward() as local_features.  Not with use_video.  Not reference fields: a JSON written
    # without them loads with the defaults (off).  mel_window K > 0: local_conv is a conv over 2 K + 1
    # frames, K on each side, the edge frames repeated past the clip's ends; 0: the 1 x 1 conv.  Needs use_mel.
    use_mel: bool = False
    mel_bins: int = 80
    mel_fft: int = 1024
    mel_hop: int = 256
    mel_fmin: float = 0.0
    mel_fmax: Optional[float] = None
    mel_window: int = 0
    # mel_f0: two more local channels behind the mel bins -- a continuous log2(F0 / sqrt(f0_min f0_max))
    # of the YIN track searched between f0_min and f0_max Hz at the mel frames, and its voiced flag
    # (ops.local_features).  Needs use_mel.
    mel_f0: bool = False
    f0_min: float = 60.0
    f0_max: float = 500.0

    # pre-emphasis of the training audio (WavFolderLoader(preemphasis=a)): the front end quantises
    # (vn[k] - a vn[k-1]) / (1 + a) of the normalised waveform, the checkpoint records a, and everything that turns the
    # model's classes back into audio (the sample logger, synthesize) runs the inverse filter.  0: off.  Not a reference
    # field: a JSON written without it loads with the default.
    preemphasis: float = 0.0

    scheduler: Optional[str] = "OneCycleLR"
    lr_pct_start: float = 0.45
    base_learning_rate: float = 0.0003
    scheduler_step_size_up: int = 1000
    scheduler_step_size_down: Optional[int] = None
    scheduler_cyclic_mode: str = "triangular"
    scheduler_cyclic_gamma: float = 1.0
    scheduler_cycle_momentum: bool = False
    max_learning_rate: float = 0.003
    scheduler_step_size: int = 10
    scheduler_step_gamma: float = 0.1
    scheduler_milestones: Optional[List[int]] = None

    dist_backend: Optional[str] = None
    dist_port: str = "8888"

    pretrained_model_path: Optional[Path] = None
    # resuming.  resume_from: a checkpoint of this run to go on from -- weights, optimizer, scheduler,
    # generators, epoch and batch position -- or "auto": <model_output_path>/checkpoints/last.ckpt if there is one, a
    # fresh run if not.  checkpoint_every_n_steps N > 0: also rewrite last.ckpt after every N-th optimizer step (0: only
    # at the end of an epoch).  Not reference fields: a JSON written without them loads with the defaults (off).
    resume_from: Optional[str] = None
    checkpoint_every_n_steps: int = 0
    model_output_path: Path = Path("models")
    tensorboard_dir: Path = Path("tensorboard_logs")
    log_samples_every: Optional[int] = None

    def to_dict(self) -> dict:
        d = asdict(self)
        for k, v in d.items():
            if isinstance(v, Path):
                d[k] = str(v)
        return d

    def to_json(self, **kw) -> str:
        return json.dumps(self.to_dict(), **kw)

    @classmethod
    def from_json(cls, text: str) -> "TrainingConfig":
        d = json.loads(text)
        d["model_config"] = ModelConfig(**d["model_config"])
        for k in ("pretrained_model_path", "model_output_path", "tensorboard_dir"):
            if d.get(k) is not None:
                d[k] = Path(d[k])
        known = {f.name for f in fields(cls)}
        return cls(**{k: v for k, v in d.items() if k in known})


def _flag(x) -> bool:
    return bool(int(x))


def check_score_pitch(score_pitch, score_samples, use_mel) -> None:
    """ValueError where --score_pitch stands without what it adds its figures to."""
    if score_pitch and not (score_samples and use_mel):
        raise ValueError("--score_pitch 1 needs --score_samples 1 --use_mel 1: the pitch figures go beside the log-mel "
                         "distance of a copy-synthesis")


def _opt_path(x):
    return None if x is None or x == "" else Path(x)


def arg_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser()
    a = p.add_argument
    a("--dataset", type=str)
    a("--batch_size", type=int, default=3)
    a("--val_batch_size", type=int, default=3)
    a("--optimizer", type=str, default="AdamW")
    a("--learning_rate", type=float, default=0.001)
    a("--momentum", type=float, default=0.9)
    a("--weight_decay", type=float, default=0.000)
    a("--scheduler", type=str, default=None)
    a("--lr_pct_start", type=float, default=0.45)
    a("--base_learning_rate", type=float, default=0.0003)
    a("--scheduler_step_size_up", type=int, default=1000)
    a("--scheduler_step_size_down", type=int, default=None)
    a("--scheduler_cyclic_mode", type=str, default="triangular")
    a("--scheduler_cyclic_gamma", type=float, default=1.0)
    a("--scheduler_cycle_momentum", type=_flag, default=False)
    a("--max_learning_rate", type=float, default=0.003)
    a("--scheduler_step_size", type=int, default=10)
    a("--scheduler_step_gamma", type=float, default=0.1)
    a("--scheduler_milestones", type=lambda x: [int(i) for i in json.loads(x)], default=None)
    a("--accumulation_steps", type=int, default=1)
    a("--num_workers", type=int, default=1)
    a("--val_num_workers", type=int, default=1)
    a("--pin_memory", type=_flag, default=False)
    a("--generate_n_samples", type=lambda x: x if x is None else int(x), default=None)
    a("--generate_temperature", type=float, default=1.0)
    a("--generate_sampling", type=str, default="reference", choices=["reference", "model"])
    a("--generate_top_k", type=int, default=0)
    a("--generate_top_p", type=float, default=1.0)
    a("--generate_temperature_sweep", type=lambda x: [float(t) for t in x.split(",") if t.strip()], default=[])
    a("--loss_rule", type=str, default="reference", choices=["reference", "model"])
    a("--ema_decay", type=float, default=0.0)
    a("--ema_warmup", type=_flag, default=True)
    a("--score_samples", type=_flag, default=False)
    a("--score_pitch", type=_flag, default=False)
    a("--clip_length", type=str, default="resample", choices=["resample", "native", "window"])
    a("--window_gain", type=str, default="file", choices=["file", "window"])
    a("--audio_rate", type=int, default=16000)
    a("--use_mel", type=_flag, default=False)
    a("--mel_bins", type=int, default=80)
    a("--mel_fft", type=int, default=1024)
    a("--mel_hop", type=int, default=256)
    a("--mel_fmin", type=float, default=0.0)
    a("--mel_fmax", type=float, default=None)
    a("--mel_window", type=int, default=0)
    a("--mel_f0", type=_flag, default=False)
    a("--f0_min", type=float, default=60.0)
    a("--f0_max", type=float, default=500.0)
    a("--preemphasis", type=float, default=0.0)
    a("--n_epochs", type=int, default=10)
    a("--n_steps_per_epoch", type=int, default=None)
    a("--use_video", type=_flag, default=True)
    a("--use_global", type=_flag, default=False)
    a("--bf16_video", type=_flag, default=False)
    a("--generate_guidance", type=float, default=1.0)
    a("--global_dropout", type=float, default=0.0)
    a("--video_antialias", type=_flag, default=False)
    a("--batch_subsample_frac", type=float, default=None)
    a("--val_batch_subsample_frac", type=float, default=None)
    a("--gradient_clipping", type=float, default=0.0)
    a("--checkpoint_every", type=int, default=1)
    a("--input_channels", type=int, default=16)
    a("--residual_channels", type=int, default=16)
    a("--skip_channels", type=int, default=8)
    a("--layer_size", type=int, default=3)
    a("--stack_size", type=int, default=3)
    a("--dist_backend", type=str, default="nccl")
    a("--dist_port", type=str, default="8888")
    a("--pretrained_model_path", type=_opt_path, default=None)
    a("--pretrained_run_exp_name", type=lambda x: None if x is None or x == "" else x, default=None)
    a("--resume_from", type=lambda x: None if x is None or x == "" else x, default=None)
    a("--checkpoint_every_n_steps", type=int, default=0)
    a("--model_output_path", type=Path,
      default=Path("models") / datetime.now().strftime("%Y%m%d%H%M%S"))
    a("--training_logs_path", type=Path, default=Path("training_logs"))
    a("--grid_user_name", type=str, default="")
    a("--grid_api_key", type=str, default="")
    a("--logger", default=None, type=str, choices=["wandb"])
    a("--log_samples_every", type=int, default=None)
    a("--log_video", type=_flag, default=False)
    a("--wandb_api_key", type=str, default="")
    a("--wandb_project", type=str, default="dance2music-pl-testing")
    # Lightning's Trainer(precision=...): 32 (exact fp32, the default) or bf16 (mixed precision,
    # Trainer's docstring); passed to train_model, not part of TrainingConfig
    a("--precision", type=_precision, default=32, choices=[32, "bf16"])
    return p


def _precision(x):
    return 32 if x == "32" else x


def check_mel_f0(mel_f0, use_mel, f0_min, f0_max) -> None:
    """ValueError where --mel_f0 stands without the frames it rides on, or with a search range that is none."""
    if not mel_f0:
        return
    if not use_mel:
        raise ValueError("--mel_f0 1 needs --use_mel 1: the F0 channels go behind the log-mel frames")
    if not 0.0 < float(f0_min) < float(f0_max) < float("inf"):
        raise ValueError(f"--f0_min and --f0_max must be finite with 0 < f0_min < f0_max, got {f0_min} and {f0_max}")


def config_from_args(args) -> TrainingConfig:
    copied = (
        "batch_size val_batch_size checkpoint_every optimizer learning_rate momentum scheduler "
        "lr_pct_start base_learning_rate scheduler_step_size_up scheduler_step_size_down "
        "scheduler_cyclic_mode scheduler_cyclic_gamma scheduler_cycle_momentum max_learning_rate "
        "scheduler_step_size scheduler_step_gamma scheduler_milestones weight_decay "
        "generate_n_samples generate_temperature generate_sampling generate_top_k generate_top_p generate_temperature_sweep loss_rule ema_decay ema_warmup score_samples clip_length audio_rate window_gain use_mel mel_bins mel_fft mel_hop mel_fmin mel_fmax preemphasis accumulation_steps num_workers val_num_workers "
        "pin_memory n_epochs n_steps_per_epoch use_video use_global bf16_video generate_guidance global_dropout video_antialias batch_subsample_frac "
        "val_batch_subsample_frac dist_backend dist_port model_output_path log_samples_every"
    ).split()
    kw = {k: getattr(args, k) for k in copied}  # NB: gradient_clipping is not among them (Q11)
    mel_window = int(getattr(args, "mel_window", 0) or 0)  # (getattr: a namespace built before the flag existed)
    if mel_window < 0 or mel_window > 16:
        raise ValueError(f"--mel_window must lie in [0, 16], got {mel_window}")
    if mel_window and not kw["use_mel"]:
        raise ValueError(f"--mel_window {mel_window} needs --use_mel 1: there are no frames to take a window of")
    score_pitch = bool(getattr(args, "score_pitch", False))  # (getattr: a namespace built before the flag existed)
    check_score_pitch(score_pitch, kw["score_samples"], kw["use_mel"])
    mel_f0 = bool(getattr(args, "mel_f0", False))  # (getattr: a namespace built before the flags existed)
    f0_min, f0_max = float(getattr(args, "f0_min", 60.0)), float(getattr(args, "f0_max", 500.0))
    check_mel_f0(mel_f0, kw["use_mel"], f0_min, f0_max)
    return TrainingConfig(
        model_config=ModelConfig(
            input_channels=args.input_channels, residual_channels=args.residual_channels,
            skip_channels=args.skip_channels, layer_size=args.layer_size,
            stack_size=args.stack_size),
        pretrained_model_path=(args.pretrained_model_path
                               if args.pretrained_model_path and args.pretrained_run_exp_name
                               else None),
        tensorboard_dir=args.training_logs_path,
        # (getattr: an argument namespace built before the flags existed)
        resume_from=getattr(args, "resume_from", None),
        checkpoint_every_n_steps=int(getattr(args, "checkpoint_every_n_steps", 0) or 0),
        mel_window=mel_window,
        score_pitch=score_pitch,
        mel_f0=mel_f0, f0_min=f0_min, f0_max=f0_max,
        **kw,
    )
