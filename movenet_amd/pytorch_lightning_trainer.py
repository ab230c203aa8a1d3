"""Trainer entry point: the counterpart of
/root/reference/movenet/pytorch_lightning_trainer.py.

    python -m movenet_amd.pytorch_lightning_trainer --dataset synthetic://clips=8,frames=8000 \
        --use_video 0 --input_channels 64 --residual_channels 16 --skip_channels 16 \
        --layer_size 2 --stack_size 2 --batch_size 2 --n_epochs 1

Same ``Dance2Music`` / ``train_model`` / CLI surface (:24-267 there): same loss
(``cross_entropy`` applied to the model's PROBABILITIES; ``--loss_rule model``
trains on ``cross_entropy`` of the logits instead), same
accuracy, same optimizer and scheduler factories and kwargs, schedulers stepped
per optimizer step.  pytorch_lightning is not available offline, so the loop
that ``Trainer.fit`` would run is written out in ``Trainer`` below with the
constructor arguments the reference passes (:233-243).  Multi-GPU is plain data
parallel over clips (movenet_amd/parallel.py) when launched with torchrun.
"""
from __future__ import annotations

import contextlib
import json
import math
import os
import time
from dataclasses import asdict
from pathlib import Path
from typing import Optional

import torch
import torch.nn as nn

from . import checkpoint
from .config import TrainingConfig, arg_parser, check_mel_f0, check_score_pitch, config_from_args
from .dataset import get_dataloader, training_contexts
from .optim import FlatAdamW, order_like_backward
from .generation import HostWords
from .utils.host import cap_torch_threads
from .parallel import FlatGradSync, contiguous_grad_span, init_distributed
from .wavenet import WaveNet


class Dance2Music(nn.Module):
    def __init__(self, dataset_fp: str, config: TrainingConfig):
        super().__init__()
        self.learning_rate = config.learning_rate
        self.dataset_fp = dataset_fp
        self.config = config
        # --use_global 1: the sorted context folders of the TRAINING set are the classes of the model's global embedding
        self.global_classes = self._class_map() if getattr(config, "use_global", False) else []
        # --use_mel 1: local conditioning on the batch's own log-mel frames
        self.use_mel = bool(getattr(config, "use_mel", False))  # (a config pickled before the field existed)
        if self.use_mel and config.use_video:
            raise ValueError("--use_mel 1 cannot be combined with --use_video 1: one local context at a time")
        local = {}
        # --mel_window K: local_conv sees K frames on each side of a frame; 0: the 1 x 1 conv
        self.mel_window = int(getattr(config, "mel_window", 0))  # (a config pickled before the field existed)
        if self.mel_window and not self.use_mel:
            raise ValueError(f"--mel_window {self.mel_window} needs --use_mel 1: there are no frames to take a window of")
        # --score_pitch 1: the pitch figures of each logged batch beside its log-mel distance
        self.score_pitch = bool(getattr(config, "score_pitch", False))  # (a config pickled before the field existed)
        check_score_pitch(self.score_pitch, getattr(config, "score_samples", False), self.use_mel)
        # --mel_f0 1: a continuous log-F0 and its voiced flag behind the mel bins
        self.mel_f0 = bool(getattr(config, "mel_f0", False))  # (a config pickled before the field existed)
        check_mel_f0(self.mel_f0, self.use_mel, getattr(config, "f0_min", 60.0), getattr(config, "f0_max", 500.0))
        if self.use_mel:
            from .ops import f0_reference, mel_filterbank
            rate = int(getattr(config, "audio_rate", 16000))
            fmax = rate / 2.0 if config.mel_fmax is None else float(config.mel_fmax)
            # (the filterbank's own ValueErrors come first: nothing is built on bad settings)
            self.mel_fbank = torch.from_numpy(mel_filterbank(int(config.mel_bins), int(config.mel_fft), rate,
                                                             float(config.mel_fmin), fmax)).to(torch.float32)
            self.local_conditioning = {"local_channels": int(config.mel_bins), "local_hop": int(config.mel_hop),
                                       "mel_fft": int(config.mel_fft), "mel_fmin": float(config.mel_fmin),
                                       "mel_fmax": fmax, "audio_rate": rate}
            local = {"local_channels": int(config.mel_bins), "local_hop": int(config.mel_hop)}
            if self.mel_window:  # (the record carries the key only then: a K = 0 run writes the file it wrote before)
                self.local_conditioning["local_window"] = self.mel_window
                local["local_window"] = self.mel_window
            if self.mel_f0:  # (likewise: a --mel_f0 0 run writes the file it wrote before)
                f_min, f_max = float(config.f0_min), float(config.f0_max)
                self.local_conditioning["f0"] = {"f_min": f_min, "f_max": f_max, "f_ref": f0_reference(f_min, f_max)}
                local["local_channels"] = checkpoint.local_channels_of(self.local_conditioning)  # (the mel bins + 2)
        self.model = WaveNet(**asdict(config.model_config), global_classes=len(self.global_classes), **local)
        if self.use_mel:  # (what checkpoint.load_into leaves there: WaveNet.spectral_distance reads the mel settings)
            self.model.local_conditioning = dict(self.local_conditioning)
        self.model.generate_sampling = config.generate_sampling  # (ValueError for an unknown rule)
        self.model.generate_top_k = config.generate_top_k        # (... a negative k, a p outside (0, 1])
        self.model.generate_top_p = config.generate_top_p
        self.model.loss_rule = getattr(config, "loss_rule", "reference")  # (a config pickled before the field existed)
        # classifier-free guidance: the scale of the logged samples, and label dropout on train steps --
        # its mask comes from a host generator of its own, seeded from the run's seed (no draw from torch's)
        if float(getattr(config, "generate_guidance", 1.0)) != 1.0:
            self.model.generate_guidance = float(config.generate_guidance)  # (ValueError without global classes)
        self.model.global_dropout = float(getattr(config, "global_dropout", 0.0))
        # --preemphasis A: the loader's front end emphasises, the model remembers A for whoever turns its classes into audio
        self.model.preemphasis = float(getattr(config, "preemphasis", 0.0))  # (ValueError outside [0, 1))
        self.model.global_dropout_generator = torch.Generator().manual_seed(torch.initial_seed() & (2 ** 63 - 1))
        self.current_epoch = 0
        self.precision = 32
        self.rank, self.world_size = 0, 1
        self.logged_raw = {}  # name -> 0-dim device tensor or float, as logged (no host sync)
        self.ema_optimizer = None  # the FlatAdamW that keeps the weights' average (--ema_decay > 0), else None

    @property
    def device(self) -> torch.device:
        return next(self.model.parameters()).device

    @property
    def logged(self) -> dict:
        """The logged values as floats.  Reading this waits for the GPU; ``log`` does not."""
        return {k: float(v) for k, v in self.logged_raw.items()}

    def log(self, name: str, value, batch_size: Optional[int] = None) -> None:
        self.logged_raw[name] = value.detach() if torch.is_tensor(value) else float(value)

    def forward(self, audio, video, **kwargs):
        return self.model(audio, video, **kwargs)

    def mel_features(self, audio, lengths=None):
        """The local features of a one-hot batch on the device, no gradient (``ops.local_features`` of its class
        indices under the run's ``local_conditioning`` record): the (B, mel_bins, T // mel_hop + 1) log-mel frames,
        with ``--mel_f0 1`` the two F0 channels behind them; None without ``--use_mel``.  ``lengths``: the batch's."""
        if not self.use_mel:
            return None
        from .ops import local_features
        extra = {} if lengths is None else {"lengths": lengths}
        return local_features(audio.argmax(1).to(torch.int32), self.config.model_config.input_channels,
                              self.local_conditioning, preemphasis=self.model.preemphasis, **extra)

    def _class_map(self):
        names = training_contexts(self.dataset_fp)
        if not names:
            raise ValueError(f"use_global: {self.dataset_fp} has no training contexts")
        return names

    def class_indices(self, contexts):
        """``Batch.contexts`` names -> the (B,) class tensor ``forward`` takes as ``global_features`` (None when the
        model has no global classes); a name the training set lacks is a ValueError that names it."""
        if not self.global_classes:
            return None
        where = {name: i for i, name in enumerate(self.global_classes)}
        unknown = sorted({str(n) for n in contexts if n not in where})
        if unknown:
            raise ValueError(f"context {unknown[0]!r} is not among the training set's classes {self.global_classes}")
        return torch.tensor([where[n] for n in contexts], dtype=torch.int64)

    def averaged_weights(self):
        """Context: the model runs on the averaged weights (``FlatAdamW.averaged_parameters``) -- a no-op without
        ``--ema_decay``, and inside a caller's own ``averaged_parameters()`` (the validation loop)."""
        opt = self.ema_optimizer
        if opt is None or opt.inside_average:
            return contextlib.nullcontext()
        return opt.averaged_parameters()

    def _generates_now(self) -> bool:
        return (self.config.log_samples_every is not None
                and (self.current_epoch + 1) % self.config.log_samples_every == 0)

    def _sample_outputs(self, audio, video, labels, lengths=None, feats=None) -> dict:
        """A step's ``generated_output`` for the sample logger -- ``generate`` on the averaged weights when there are
        any -- and, with ``--score_samples 1`` on a step that generates, the clips' scores under ``"sample_scores"`` (a
        key that is absent otherwise).  (The views are swapped only on a step that generates; the step's autograd graph
        holds the parameters themselves, which point into the raw buffer again before ``backward`` runs.)"""
        with (self.averaged_weights() if self._generates_now() else contextlib.nullcontext()):
            # (which keeps the epoch gate: None on the other epochs; the features only where the model takes them)
            gen = self.generate(audio, video, labels, **({} if feats is None else {"local_features": feats}))
            out = {"generated_output": gen}
            if gen is not None and getattr(self.config, "score_samples", False):
                # (the call without lengths is the call it was: the argument goes only where the batch has lengths)
                out["sample_scores"] = self.score_samples(gen, audio, video, labels,
                                                          **({} if lengths is None else {"lengths": lengths}),
                                                          **({} if feats is None else {"local_features": feats}))
            if gen is not None and lengths is not None:
                # the logger prompts from a clip's first RF samples: clips shorter than that are left out of its rows
                out["prompt_ok"] = [int(n) >= self.model.receptive_fields for n in lengths]
        return out

    def score_samples(self, generated, audio, video, labels=None, lengths=None, local_features=None) -> dict:
        """bits per sample of the generated clips and of the clips they were prompted from, each under the clip's own
        conditioning (video, label; temperature 1, no guidance: the model's own distribution), from ONE
        ``WaveNet.score`` call: the generated rows (len(sweep) per clip, clip-major, under a temperature sweep), then
        the sources.  A generated length other than the source's is scored over the common leading part.  With
        ``lengths`` (the batch's, clip_length="native") a source is scored over its own real samples only; the
        generated rows are scored in full.  With ``local_features`` (``--use_mel 1``) also ``mel_distance_db`` and
        ``mel_l1``, one value per generated row: its log-mel distance from its source clip."""
        n = generated.shape[0] // audio.shape[0]
        frames = min(int(generated.shape[2]), int(audio.shape[2]))
        if video is not None and frames != int(audio.shape[2]):
            raise ValueError("--score_samples with a video context needs generate_n_samples to be the clips' length")

        def both(per_clip):
            return None if per_clip is None else torch.cat([per_clip.repeat_interleave(n, dim=0), per_clip])
        # (--use_mel: a generated clip is scored under the features it was generated under -- its source clip's)
        mel = {} if local_features is None else {"local_features": both(local_features)}
        res = self.model.score(torch.cat([generated[:, :, :frames], audio[:, :, :frames].to(generated.dtype)]),
                               both(video), both(labels), **mel,
                               lengths=None if lengths is None else
                               [frames] * int(generated.shape[0]) + [min(int(v), frames) for v in lengths])
        bits = res.bits_per_sample.detach()
        out = {"bits_per_sample": bits[:generated.shape[0]], "source_bits_per_sample": bits[generated.shape[0]:]}
        if local_features is not None:
            # --use_mel: the clip is a copy-synthesis of its source, so the two can be compared -- the log-mel distance
            # of each generated row from the clip it was prompted from, over the frames past the prompt and inside the
            # clip's own length (WaveNet.spectral_distance)
            clip_len = [frames] * int(audio.shape[0]) if lengths is None else [min(int(v), frames) for v in lengths]
            gen_idx = generated[:, :, :frames].argmax(1)
            src_idx = audio[:, :, :frames].argmax(1).repeat_interleave(n, dim=0)
            row_len = [v for v in clip_len for _ in range(n)]
            dist = self.model.spectral_distance(gen_idx, src_idx, lengths=row_len)
            out["mel_distance_db"], out["mel_l1"] = dist.lsd_db, dist.l1
            if self.score_pitch:
                # --score_pitch 1: the pitch track of each generated row against its source's, over the same kind of
                # span (WaveNet.pitch_distance); a rate is NaN where its denominator is 0
                pd = self.model.pitch_distance(gen_idx, src_idx, lengths=row_len)
                out["f0_rmse_cents"] = torch.where(pd.voiced_frames > 0, pd.f0_rmse_cents,
                                                   torch.full_like(pd.f0_rmse_cents, float("nan")))
                out["vuv_error_rate"] = pd.vuv_errors.double() / pd.frames.double()
                out["gross_pitch_error_rate"] = pd.gross_errors.double() / pd.voiced_frames.double()
        return out

    def generate(self, audio, video, labels=None, local_features=None):
        if not self._generates_now():
            return None
        sweep = list(getattr(self.config, "generate_temperature_sweep", None) or ())
        n = len(sweep)

        def rows(t):  # every clip once per temperature, clip-major, in ONE generate() call (LogSamplesCallback's layout)
            return t if t is None or not sweep else t.repeat_interleave(n, dim=0)
        # (--use_mel: generate() keeps the reference's signature, so the frames go in through the model's setting, which
        # the call uses up)
        if local_features is not None:
            self.model.generate_local_features = rows(local_features)
        return self.model.generate(
            rows(audio), rows(video), rows(labels), n_samples=self.config.generate_n_samples,
            temperature=sweep * audio.shape[0] if sweep else self.config.generate_temperature).detach()

    def _shared_step(self, batch, prefix: str):
        audio, video, contexts, fps, info = batch
        # ("bf16": the one-hot batch is exact in bfloat16; the model takes the class indices from it)
        dtype = torch.bfloat16 if self.precision == "bf16" else getattr(torch, f"float{self.precision}")
        audio = audio.type(dtype).to(self.device)
        if self.config.use_video:
            # (bf16 with video, Trainer(bf16_video=True): the encoder and up-sampler stay fp32, and so does their input)
            video = video.type(torch.float32 if self.precision == "bf16" else dtype).to(self.device)
        # output = self(audio, video) (probabilities, Q1); target = audio[:, :, RF:].argmax(1);
        # loss = cross_entropy(output, target) on those probabilities (Q2); accuracy -- the
        # reference's lines 62-66 as ONE autograd node: softmax + loss + accuracy in one pass
        # over the head's logits, their gradient in one pass back (ops.wavenet_forward_loss)
        # (through both modules' __call__, like the reference's self(audio, video): forward
        # hooks and overrides keep firing)
        labels = self.class_indices(contexts)  # (None without --use_global)
        extra = {} if labels is None else {"global_features": labels}
        lengths = getattr(batch, "lengths", None)  # (real samples per row: WavFolderLoader(clip_length="native"))
        if lengths is not None:
            from .ops import valid_columns
            extra["lengths"] = lengths = [int(v) for v in lengths]
            T, rf = int(audio.shape[2]), self.model.receptive_fields
            # host arithmetic on the loader's host list: no synchronisation
            self.log(f"{prefix}_valid_frac", sum(valid_columns(lengths, T, rf)) / max(len(lengths) * (T - rf), 1),
                     batch_size=self.config.batch_size)
        feats = self.mel_features(audio, lengths)  # (None without --use_mel)
        if feats is not None:
            extra["local_features"] = feats
        loss, acc, output = self(audio, video if self.config.use_video else None, return_loss=True, **extra)
        self.log(f"{prefix}_loss", loss, batch_size=self.config.batch_size)
        self.log(f"{prefix}_acc", acc, batch_size=self.config.batch_size)
        if self.model.loss_rule == "model":  # the loss is a likelihood in nats: also in bits (a device scalar, no sync)
            self.log(f"{prefix}_bits_per_sample", loss.detach() / math.log(2.0), batch_size=self.config.batch_size)
        return loss, output, audio, video, labels, lengths, feats

    def training_step(self, batch, batch_idx):
        if self.model.global_dropout > 0:
            # (generate() leaves the model in eval mode, as the reference's does: with samples logged on train steps the
            # rest of the epoch would run without label dropout, which forward applies in train mode only)
            self.model.train()
        loss, output, audio, video, labels, lengths, feats = self._shared_step(batch, "train")
        return {"loss": loss, "output": output.detach(), **self._sample_outputs(audio, video, labels, lengths, feats)}

    def validation_step(self, batch, batch_idx):
        _, output, audio, video, labels, lengths, feats = self._shared_step(batch, "val")
        return {"output": output.detach(), **self._sample_outputs(audio, video, labels, lengths, feats)}

    def _loader(self, train: bool):
        c = self.config
        return get_dataloader(
            self.dataset_fp, input_channels=c.model_config.input_channels,
            batch_size=c.batch_size if train else c.val_batch_size, train=train,
            rank=self.rank, world_size=self.world_size, shuffle=train, pin_memory=c.pin_memory,
            num_workers=c.num_workers if train else c.val_num_workers, use_video=c.use_video,
            batch_subsample_frac=c.batch_subsample_frac if train else c.val_batch_subsample_frac,
            # raw uint8 frames of a WAV folder: the GPU front end's resize rule (getattr: a config pickled before the
            # field existed)
            video_antialias=bool(getattr(c, "video_antialias", False)),
            clip_length=getattr(c, "clip_length", "resample"), audio_rate=int(getattr(c, "audio_rate", 16000)),
            window_gain=getattr(c, "window_gain", "file"),
            # (--preemphasis: the keyword goes only where it is on, the call without it is the call it was)
            **({"preemphasis": self.model.preemphasis} if self.model.preemphasis > 0 else {}),
            # row F2: class indices cross PCIe (4 bytes per sample), the (B,Q,T) one-hot the Batch
            # contract asks for is formed on the device
            device=self.device if self.device.type == "cuda" else None)

    def train_dataloader(self):
        print("using full audio samples." if self.config.batch_subsample_frac is None
              else f"using {self.config.batch_subsample_frac} of audio samples.")
        return self._loader(True)

    def val_dataloader(self):
        return self._loader(False)

    def configure_optimizers(self):
        c = self.config
        base = {"lr": self.learning_rate, "weight_decay": c.weight_decay}
        opt_kw = {"Adam": base, "AdamW": base, "SGD": {**base, "momentum": c.momentum},
                  "RMSprop": {**base, "momentum": c.momentum}}
        if c.optimizer not in opt_kw:
            raise ValueError(f"optimizer {c.optimizer} not recognized. "
                             f"Must be one of {opt_kw.keys()}")
        ema_decay = float(getattr(c, "ema_decay", 0.0))  # (a config pickled before the fields existed)
        flat = c.optimizer in ("Adam", "AdamW") and self.device.type == "cuda"
        if ema_decay > 0 and not flat:
            raise ValueError(f"--ema_decay {ema_decay:g} needs the fused Adam / AdamW step on a GPU (the average is "
                             f"kept by its kernel); optimizer {c.optimizer} on {self.device.type} has none")
        self.ema_optimizer = None
        if flat:
            # same update rule as torch.optim.Adam / AdamW, one HIP kernel over one flat buffer
            # (labels train the layers' context convs too: their gradients sit where a video-conditioned run's do)
            optimizer = FlatAdamW(order_like_backward(self.model, bool(c.use_video) or bool(self.global_classes) or self.use_mel), decoupled=c.optimizer == "AdamW",
                                  ema_decay=ema_decay, ema_warmup=bool(getattr(c, "ema_warmup", True)),
                                  **opt_kw[c.optimizer])
            self.ema_optimizer = optimizer if ema_decay > 0 else None
        else:
            optimizer = getattr(torch.optim, c.optimizer)(self.model.parameters(), **opt_kw[c.optimizer])
        print(f"using optimizer: {optimizer}")
        optimizers = {"optimizer": optimizer}
        if c.scheduler is not None:
            n_updates = math.ceil(len(self._loader(True)) / c.accumulation_steps)
            sched_kw = {
                "OneCycleLR": dict(max_lr=c.max_learning_rate, epochs=c.n_epochs,
                                   steps_per_epoch=n_updates, pct_start=c.lr_pct_start,
                                   three_phase=True),
                "CyclicLR": dict(base_lr=c.base_learning_rate, max_lr=c.max_learning_rate,
                                 step_size_up=c.scheduler_step_size_up,
                                 step_size_down=c.scheduler_step_size_down,
                                 mode=c.scheduler_cyclic_mode, gamma=c.scheduler_cyclic_gamma,
                                 cycle_momentum=c.scheduler_cycle_momentum),
                "StepLR": dict(step_size=c.scheduler_step_size, gamma=c.scheduler_step_gamma),
                "MultiStepLR": dict(milestones=c.scheduler_milestones,
                                    gamma=c.scheduler_step_gamma),
            }
            if c.scheduler not in sched_kw:
                raise ValueError(f"scheduler {c.scheduler} not recognized. "
                                 f"Must be one of {sched_kw.keys()}")
            optimizers["lr_scheduler"] = {
                "scheduler": getattr(torch.optim.lr_scheduler, c.scheduler)(
                    optimizer, **sched_kw[c.scheduler]),
                "interval": "step",
            }
            print(f"using scheduler: {optimizers['lr_scheduler']}")
        return optimizers


class _DeferredRecord:
    """One optimizer step's log record whose tensor values are still being computed.  The device
    scalars are gathered into one tensor and published to pinned host memory by a kernel queued
    behind them (generation.HostWords); ``resolve()`` -- called a step later -- polls for it.
    (``float(tensor)`` is a synchronous copy on the current stream: it waits for everything
    enqueued so far, i.e. it would serialise the host's enqueueing of step k + 1 with the GPU's
    execution of it.)"""

    def __init__(self, rec: dict):
        self.rec = rec
        self.keys = [k for k, v in rec.items() if torch.is_tensor(v)]
        self.token, self.host = None, None
        if self.keys:
            vals = torch.stack([rec[k].detach().to(torch.float32).reshape(()) for k in self.keys])
            if vals.is_cuda:
                self.token = HostWords.publish(vals)
            else:
                self.host = vals.tolist()

    def resolve(self) -> dict:
        out = dict(self.rec)
        if self.keys:
            out.update(zip(self.keys, HostWords.read(self.token) if self.token is not None else self.host))
        return out


class Trainer:
    """The part of ``pytorch_lightning.Trainer.fit`` the reference relies on."""

    def __init__(self, max_epochs: int, default_root_dir=None, gradient_clip_val: Optional[float] = 0.0,
                 accumulate_grad_batches: int = 1, logger=None, log_every_n_steps: int = 1,
                 num_sanity_val_steps: int = 0, callbacks=None, track_grad_norm: int = 2,
                 limit_train_batches: Optional[int] = None, device: Optional[str] = None,
                 enable_checkpointing: bool = True, limit_val_batches: Optional[int] = None,
                 precision=32, bf16_video: bool = False, checkpoint_every_n_steps: int = 0):
        # bf16_video: with precision="bf16", train a use_video model too -- the conditioned layers on bf16 operands
        # (WaveNet.bf16_context, which fit() sets and leaves set); ValueError with precision=32.
        # Lightning's precision switch: 32 (default) trains in exact fp32; "bf16" runs the layer stack's
        # products on bf16 operands with fp32 accumulation (WaveNet.forward_precision = "bf16"), fp32
        # everywhere else -- master weights, optimizer, head and loss included.  fit() then SETS, and leaves set,
        # model.model.forward_precision = "bf16" and, on a model with class labels (--use_global), model.model.global_path
        # = "bias": the model keeps both after training (reset them for an fp32 use with video, which "bias" refuses)
        # checkpoint_every_n_steps N > 0: after every N-th optimizer step checkpoints/last.ckpt is rewritten with the
        # run's position inside the epoch (no epoch=... file); 0: checkpoints at the end of an epoch only.
        if precision in (16, "16", "16-mixed"):
            raise NotImplementedError("precision=16 (fp16 training) needs loss scaling, which movenet_amd "
                                      "does not implement; use precision='bf16' or 32")
        if precision not in (32, "32", "bf16"):
            raise ValueError(f"precision must be 32 or 'bf16', got {precision!r}")
        self.precision = 32 if precision in (32, "32") else "bf16"
        self.bf16_video = bool(bf16_video)
        if self.bf16_video and self.precision != "bf16":
            raise ValueError("Trainer(bf16_video=True) needs precision='bf16'")
        self.max_epochs = max_epochs
        self.root = Path(default_root_dir) if default_root_dir is not None else None
        self.clip = gradient_clip_val or 0.0
        self.accum = max(1, accumulate_grad_batches)
        self.log_every = max(1, log_every_n_steps)
        self.track_grad_norm = track_grad_norm
        self.limit = limit_train_batches
        # (Lightning's limit_val_batches; default: the training limit, as before)
        self.limit_val = limit_val_batches if limit_val_batches is not None else limit_train_batches
        self.epoch_seconds = []  # wall time of each epoch's training loop
        self.device = device
        self.checkpointing = enable_checkpointing
        self.checkpoint_every_n_steps = max(0, int(checkpoint_every_n_steps or 0))
        self.callbacks = list(callbacks or [])
        self.current_epoch = 0
        self.rank = 0
        self.history = []      # one dict per optimizer step
        self.global_step = 0
        self.optimizer = None  # what fit() steps (its averaged_parameters() / ema_state_dict() when --ema_decay is on)

    def _hyper(self, model: "Dance2Music", world: int) -> dict:
        return checkpoint.hyper_parameters(model.config, model.dataset_fp, self.precision, self.bf16_video, self.accum,
                                           world)

    def _checked_checkpoint(self, model: "Dance2Music", ckpt_path, world: int) -> dict:
        """The checkpoint to resume from, read and checked against this run (``checkpoint.check_resumable``) with
        nothing but the host: every refusal is a ValueError raised before the device is touched."""
        obj = checkpoint.read_checkpoint(ckpt_path)
        c = model.config
        averaging = (float(getattr(c, "ema_decay", 0.0)) > 0) and c.optimizer in ("Adam", "AdamW")
        checkpoint.check_resumable(obj, ckpt_path, self._hyper(model, world), self.max_epochs, averaging,
                                   local_window=int(getattr(model, "mel_window", 0)),
                                   f0=(getattr(model, "local_conditioning", None) or {}).get("f0"))
        names = checkpoint.global_classes_of(obj)
        if names != list(model.global_classes):
            raise ValueError(f"{ckpt_path}: global_classes is {names}, but this run's training set has "
                             f"{list(model.global_classes)}")
        return obj

    def _save_checkpoint(self, model: "Dance2Music", scheduler, world: int, epoch: int, next_epoch: int,
                         batches_done: int, epoch_file: bool) -> None:
        """Rank 0's checkpoint of this moment (``checkpoint.training_checkpoint``): ``checkpoints/last.ckpt``, and at the
        end of an epoch (``epoch_file``) ``checkpoints/epoch=E-step=S.ckpt`` with the same content before it.  Both
        through a temporary file and ``os.replace``."""
        ck = self.root / "checkpoints"
        ck.mkdir(parents=True, exist_ok=True)
        obj = checkpoint.training_checkpoint(
            model, self.optimizer, scheduler, epoch=epoch, global_step=self.global_step, next_epoch=next_epoch,
            batches_done=batches_done, hyper=self._hyper(model, world), history_len=self.global_step)
        if epoch_file:
            checkpoint.write_checkpoint(obj, ck / f"epoch={epoch}-step={self.global_step}.ckpt")
        checkpoint.write_checkpoint(obj, ck / "last.ckpt")

    def fit(self, model: Dance2Music, ckpt_path=None) -> None:
        """``ckpt_path``: a checkpoint this trainer wrote (``last.ckpt``, or an ``epoch=...`` file) -- the run goes on
        from it: weights, optimizer moments and step counts, the weights' average, scheduler, the label-dropout and
        torch CPU generators, ``global_step``, and the batch of the epoch it stopped before.  Every rank
        reads the file itself.  ``history`` starts empty; its records' step numbers continue from ``global_step``."""
        if self.precision == "bf16":
            if model.config.use_video and not self.bf16_video:
                raise ValueError("Trainer(precision='bf16') trains audio-only models: set use_video to False")
            model.model.forward_precision = "bf16"
            model.precision = "bf16"
            if self.bf16_video:
                model.model.bf16_context = True
            from .ops import bf16_mode
            bf16_mode(model.model, False)  # (the channel constraint, before anything runs)
            if int(getattr(model.model, "global_classes", 0)) > 0 and not model.config.use_video:
                # labels (--use_global): the one-vector-per-layer path of the bf16 layer kernels, by name
                model.model.global_path = "bias"
        rank, world, local_rank = init_distributed(model.config.dist_backend
                                                   if torch.cuda.is_available() else "gloo",
                                                   model.config.dist_port)
        model.rank, model.world_size = rank, world
        self.rank = rank
        resumed = None if ckpt_path is None else self._checked_checkpoint(model, ckpt_path, world)
        cap_torch_threads()  # the container's CPU share, not the visible cores (utils/host.py)
        dev = torch.device(self.device) if self.device else torch.device("cuda", local_rank)
        if dev.type != "cuda":
            raise RuntimeError("movenet_amd trains on MI355X devices only (no CPU path)")
        model.to(dev)
        opt_cfg = model.configure_optimizers()
        optimizer = self.optimizer = opt_cfg["optimizer"]
        averaging = model.ema_optimizer is not None
        scheduler = opt_cfg.get("lr_scheduler", {}).get("scheduler")
        sync = FlatGradSync(model.model.parameters(), world)
        sync.broadcast_parameters(0)
        start_epoch = skip_batches = 0
        if resumed is not None:
            # the weights go INTO the storage the parameters already have (load_state_dict copies in place: with
            # FlatAdamW that storage is optimizer.flat), then the moments, step counts and the average into theirs
            model.model.load_state_dict(checkpoint._state_dict_of(resumed, ckpt_path, False), strict=True)
            optimizer.load_state_dict(resumed["optimizer_states"][0])
            if scheduler is not None:
                scheduler.load_state_dict(resumed["lr_schedulers"][0])
            where = resumed["resume"]
            gen = getattr(model.model, "global_dropout_generator", None)
            if gen is not None:
                gen.set_state(where["global_dropout_generator"])
            torch.set_rng_state(where["torch_rng"])
            self.global_step = int(resumed["global_step"])
            start_epoch, skip_batches = int(where["epoch"]), int(where["batches_done"])
        elif averaging and world > 1:
            # the average starts at the parameters every rank now holds; from here each rank forms the same average from
            # the same reduced gradients, and nothing of it is ever exchanged
            with torch.no_grad():
                optimizer.ema.copy_(optimizer.flat)
        log_f = None
        if self.root is not None and rank == 0:
            self.root.mkdir(parents=True, exist_ok=True)
            log_f = open(self.root / "metrics.jsonl", "a")
        pending = []  # records whose values are still device tensors

        def flush_records():
            """Resolve the queued records (waiting only for the step that produced them -- which
            is why a record is resolved after the NEXT step has been enqueued), append them to
            history, print / write them."""
            while pending:
                rec = pending.pop(0).resolve()
                self.history.append(rec)
                if rank == 0 and (rec["step"] + 1) % self.log_every == 0:
                    print(json.dumps(rec), flush=True)
                    if log_f:
                        log_f.write(json.dumps(rec) + "\n")
                        log_f.flush()

        saving = rank == 0 and self.root is not None and self.checkpointing
        for epoch in range(start_epoch, self.max_epochs):
            model.current_epoch = self.current_epoch = epoch
            model.train()
            loader = model.train_dataloader()
            loader.set_epoch(epoch)
            n_batches = len(loader) if self.limit is None else min(len(loader), self.limit)
            optimizer.zero_grad(set_to_none=True)
            t0 = time.perf_counter()
            batches = enumerate(loader)
            if skip_batches:
                # a resumed epoch: the batches the saved run had consumed are drawn and dropped (the loaders key their
                # draws on (seed, epoch, ...) and SyntheticLoader's crops are sequential within the epoch)
                for _ in range(skip_batches):
                    next(batches, None)
                skip_batches = 0
            for batch_idx, batch in batches:
                if batch_idx >= n_batches:
                    break
                out = model.training_step(batch, batch_idx)
                (out["loss"] / self.accum).backward()
                for cb in self.callbacks:
                    cb.on_train_batch_end(self, model, out, batch, batch_idx)
                if (batch_idx + 1) % self.accum == 0 or batch_idx + 1 == n_batches:
                    sync.sync_gradients()
                    rec = {"epoch": epoch, "step": self.global_step, **model.logged_raw}
                    used = [p for p in model.model.parameters() if p.grad is not None]
                    # every gradient is a view of ONE flat buffer (ops._run_backward): the total
                    # norm is one reduction over that span (parameters without a gradient are
                    # zero-filled gaps), not one launch per parameter; and nothing here reads a
                    # value back -- the record is resolved a step later (flush_records)
                    # (... only while the gaps really are zero: mvn_backward writes a gradient for EVERY decoder parameter
                    # into the buffer and autograd merely withholds the view of a frozen one -- its slot is a gap with
                    # data in it, which torch's clip_grad_norm_ and the reference do not count.  Then: per parameter.)
                    all_trainable = all(p.requires_grad for p in model.model.parameters())
                    span = (contiguous_grad_span(used)
                            if (self.track_grad_norm or self.clip > 0) and used and all_trainable else None)
                    if self.track_grad_norm and used:
                        if span is not None:
                            rec["grad_norm_total"] = span.norm(self.track_grad_norm)
                        else:
                            rec["grad_norm_total"] = torch.stack(
                                [p.grad.detach().norm(self.track_grad_norm) for p in used]).norm(self.track_grad_norm)
                    if self.clip > 0 and used:
                        if span is not None:  # torch.nn.utils.clip_grad_norm_'s rule on the span
                            total = (rec["grad_norm_total"] if self.track_grad_norm == 2 else span.norm(2))
                            span.mul_((self.clip / (total + 1e-6)).clamp(max=1.0))
                        else:
                            torch.nn.utils.clip_grad_norm_(model.model.parameters(), self.clip)
                    optimizer.step()
                    optimizer.zero_grad(set_to_none=True)
                    rec["lr"] = optimizer.param_groups[0]["lr"]
                    if scheduler is not None:
                        scheduler.step()
                    self.global_step += 1
                    flush_records()          # the PREVIOUS step's values: ready by now
                    pending.append(_DeferredRecord(rec))
                    if self.checkpoint_every_n_steps and self.global_step % self.checkpoint_every_n_steps == 0:
                        flush_records()  # history and metrics.jsonl hold every step the file's global_step counts
                        if saving:
                            self._save_checkpoint(model, scheduler, world, epoch, epoch, batch_idx + 1, False)
            flush_records()
            torch.cuda.synchronize(dev)
            epoch_s = time.perf_counter() - t0
            self.epoch_seconds.append(epoch_s)
            model.eval()
            # epoch means of val_loss / val_acc, weighted by batch size and summed over the
            # ranks' shards: what Lightning's self.log(..., on_epoch=True) reports for
            # validation_step (pytorch_lightning_trainer.py:91-92), not the last batch's values
            val_dev = torch.zeros(3, dtype=torch.float64, device=dev)  # loss * n, acc * n, n
            # (--ema_decay: val_loss / val_acc / val_bits_per_sample and the validation samples are the averaged weights')
            with torch.no_grad(), (optimizer.averaged_parameters() if averaging else contextlib.nullcontext()):
                for batch_idx, batch in enumerate(model.val_dataloader()):
                    if self.limit_val is not None and batch_idx >= self.limit_val:
                        break
                    out = model.validation_step(batch, batch_idx)
                    n = float(out["output"].shape[0])
                    val_dev += torch.stack([torch.as_tensor(model.logged_raw["val_loss"], device=dev).double() * n,
                                            torch.as_tensor(model.logged_raw["val_acc"], device=dev).double() * n,
                                            torch.tensor(n, dtype=torch.float64, device=dev)])
                    for cb in self.callbacks:
                        cb.on_validation_batch_end(self, model, out, batch, batch_idx, 0)
            if world > 1:
                import torch.distributed as dist
                t = val_dev if dist.get_backend() == "nccl" else val_dev.cpu()
                dist.all_reduce(t, op=dist.ReduceOp.SUM)
                val_dev = t
            val_sum = val_dev.cpu()
            if val_sum[2] > 0:
                model.logged_raw["val_loss"] = float(val_sum[0] / val_sum[2])
                model.logged_raw["val_acc"] = float(val_sum[1] / val_sum[2])
                if "val_bits_per_sample" in model.logged_raw:
                    model.logged_raw["val_bits_per_sample"] = model.logged_raw["val_loss"] / math.log(2.0)
            self.val_epoch_means = {k: v for k, v in model.logged.items() if k.startswith("val")}
            if rank == 0:
                print(json.dumps({"epoch": epoch, "epoch_seconds": epoch_s,
                                  **{k: v for k, v in model.logged.items() if k.startswith("val")}}),
                      flush=True)
                if saving:
                    # Lightning's layout: "state_dict" with the LightningModule's "model." prefix; the resumed run's
                    # next epoch is epoch + 1, none of its batches consumed
                    self._save_checkpoint(model, scheduler, world, epoch, epoch + 1, 0, True)
        if log_f:
            log_f.close()


def train_model(dataset: str, config: TrainingConfig, logger_name: Optional[str] = None,
                log_video: bool = False, wandb_project: Optional[str] = None,
                limit_train_batches: Optional[int] = None, precision=32) -> Trainer:
    # (bf16_video travels in the config: --bf16_video 1)
    model = Dance2Music(dataset, config)
    pretrained = getattr(config, "pretrained_model_path", None)
    if pretrained and getattr(config, "resume_from", None):
        raise ValueError("--pretrained_model_path starts a new run from a file's weights, --resume_from continues a "
                         "run: give one of them")
    resume = checkpoint.resolve_resume(getattr(config, "resume_from", None), config.model_output_path)
    if pretrained:
        # fine-tuning, the reference's semantics (its trainer.py:240-262): the file's weights, then a fresh optimizer,
        # a fresh scheduler and epoch 0
        names = checkpoint.global_classes_of(checkpoint.read_checkpoint(pretrained))
        if names != list(model.global_classes):
            raise ValueError(f"{pretrained}: global_classes is {names}, but this run's training set has "
                             f"{list(model.global_classes)}")
        checkpoint.load_into(model.model, pretrained, strict=True)
    if logger_name == "wandb":
        raise NotImplementedError("wandb logging is a SaaS integration and out of scope "
                                  "(SURVEY.md section 2); metrics go to <model_output_path>/metrics.jsonl")
    print("Using logger: None")
    callbacks = []
    if config.log_samples_every:
        # the reference attaches this callback only under wandb (:223-229); without wandb the
        # decoded samples go to <model_output_path>/samples/ as .wav files
        from .callbacks import LogSamplesCallback
        callbacks.append(LogSamplesCallback(log_every_n_epochs=config.log_samples_every, log_video=log_video,
                                            temperature_sweep=getattr(config, "generate_temperature_sweep", None) or (),
                                            guidance=float(getattr(config, "generate_guidance", 1.0)),
                                            preemphasis=float(getattr(config, "preemphasis", 0.0))))
    trainer = Trainer(
        max_epochs=config.n_epochs, default_root_dir=config.model_output_path,
        gradient_clip_val=config.gradient_clipping,
        accumulate_grad_batches=config.accumulation_steps, logger=None, log_every_n_steps=1,
        num_sanity_val_steps=0, callbacks=callbacks, track_grad_norm=2,
        limit_train_batches=(limit_train_batches if limit_train_batches is not None
                             else config.n_steps_per_epoch),
        precision=precision, bf16_video=bool(getattr(config, "bf16_video", False)),
        checkpoint_every_n_steps=int(getattr(config, "checkpoint_every_n_steps", 0) or 0))
    # (a fresh run makes the call it always made)
    trainer.fit(model=model, **({} if resume is None else {"ckpt_path": resume}))
    return trainer


if __name__ == "__main__":
    import logging

    logging.basicConfig(level=logging.INFO,
                        format="%(asctime)s: %(levelname)s: %(name)s: %(message)s")
    args = arg_parser().parse_args()
    train_model(args.dataset, config_from_args(args), logger_name=args.logger,
                log_video=args.log_video, wandb_project=args.wandb_project, precision=args.precision)
