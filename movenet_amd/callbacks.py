"""Sample logging without wandb (row F4 of SURVEY.md section 8).

Mirrors ``movenet.callbacks.LogSamplesCallback`` (/root/reference/movenet/callbacks.py:24-134):
same constructor, same hooks and the same epoch gate; every ``log_every_n_epochs`` epochs
the model's one-step predictions (``outputs["output"]``) and its free-running generation
(``outputs["generated_output"]``) are turned back into waveforms -- argmax over the class
axis, then mu-law decoding (:66-76) -- and logged.  The reference uploads a wandb table
with the clips resampled to the source video's rate (librosa / torchvision, both absent
offline); here the decoded waveforms are written as 16-bit PCM ``.wav`` files at the model
rate (MAX_AUDIO_FRAMES / 10 = 16 kHz) under ``<default_root_dir>/samples/<split>/`` with
one JSON line per clip in ``samples/index.jsonl`` (the table's columns).  The decoding runs
on the GPU (``mvn_mu_law_decode``: formula of RESEARCH.md:156-163, parity unpinned).

``temperature_sweep`` (default empty: off, the files and rows above unchanged): every logged clip is generated once
per temperature of the sweep -- by the module, in ONE ``generate()`` call that carries each clip len(sweep) times with
a temperature per sequence -- so ``outputs["generated_output"]`` holds len(sweep) rows per clip, clip-major.  They are
written as ``...-gen-T<value>.wav``, one index row per (clip, temperature) with a ``temperature`` field.

With ``--score_samples 1`` the module also scores each logged batch (``Dance2Music.score_samples``: one
``WaveNet.score`` call) and every row of a clip carries ``bits_per_sample`` -- of the generated clip under the
conditioning it was generated with -- and ``source_bits_per_sample`` -- of the clip it was prompted from.  Off (the
default), no row carries either key.  Under ``--use_mel 1`` the scores also hold ``mel_distance_db`` and ``mel_l1``, the
log-mel distance of each generated row from the clip it was prompted from (``WaveNet.spectral_distance``), and every
row carries them too; without ``--use_mel 1`` the rows are what they were.  ``--score_pitch 1`` (with both flags above)
adds ``f0_rmse_cents``, ``vuv_error_rate`` and ``gross_pitch_error_rate`` of the same pairs (``WaveNet.pitch_distance``,
one call per logged batch; null where a figure's denominator is 0); off, no row carries them.

With ``--ema_decay`` the module generates ``outputs["generated_output"]`` on the averaged weights
(``Dance2Music.averaged_weights``), on the train hook and on the validation hook, and the validation hook's
``outputs["output"]`` comes from them too (the whole validation loop runs on them); the train hook's
``outputs["output"]`` is the raw iterate's, like the train metrics.

With ``--preemphasis A`` (A > 0) the classes describe the pre-emphasised signal, so every file -- origin, prediction
and each generated one -- is written from ``ops.deemphasis_pcm16``: the bytes ``synthesize`` streams for the same
classes.  Every row then carries ``preemphasis``; at 0 nothing changes and no row carries the key.
"""
from __future__ import annotations

import json
import wave
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from .ops import deemphasis_pcm16, mu_law_decode
from .wavenet import MAX_AUDIO_FRAMES

COLUMNS = ["split", "epoch", "batch_idx", "fp", "origin_audio", "pred_audio", "gen_audio"]
SAMPLE_RATE = MAX_AUDIO_FRAMES // 10  # 16,000 (callbacks.py:88)


def write_wav(path: Path, waveform: np.ndarray, sample_rate: int = SAMPLE_RATE) -> None:
    """waveform in [-1, 1] -> mono 16-bit PCM."""
    pcm = (np.clip(np.asarray(waveform, dtype=np.float64), -1.0, 1.0) * 32767.0).round().astype("<i2")
    write_pcm16(path, pcm, sample_rate)


def write_pcm16(path: Path, pcm: np.ndarray, sample_rate: int = SAMPLE_RATE) -> None:
    """int16 PCM -> mono 16-bit WAV, the samples as they are."""
    pcm = np.asarray(pcm)
    if pcm.dtype != np.int16:
        raise ValueError(f"pcm must be int16, got {pcm.dtype}")
    pcm = pcm.astype("<i2", copy=False)
    path.parent.mkdir(parents=True, exist_ok=True)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sample_rate)
        w.writeframes(pcm.tobytes())


class LogSamplesCallback:
    def __init__(self, log_every_n_epochs: int = 10, log_video: bool = True, temperature: float = 1.0,
                 out_dir: Optional[str] = None, temperature_sweep=(), guidance: float = 1.0,
                 preemphasis: float = 0.0):
        self.log_every_n_epochs = log_every_n_epochs
        self.log_video = log_video  # kept for signature parity: there is no video to re-attach
        self.temperature = temperature
        self.out_dir = Path(out_dir) if out_dir is not None else None
        self.temperature_sweep = [float(t) for t in (temperature_sweep or ())]
        self.guidance = float(guidance)  # the module's classifier-free guidance scale (1.0: off, no field in the rows)
        # the run's pre-emphasis coefficient (0.0: off -- the files and rows as they were)
        self.preemphasis = float(preemphasis)
        self.columns = list(COLUMNS)

    def on_train_batch_end(self, trainer, pl_module, outputs, batch, batch_idx):
        if (trainer.current_epoch + 1) % self.log_every_n_epochs != 0:
            return
        self.log_samples("train", trainer, pl_module, outputs, batch, batch_idx)

    def on_validation_batch_end(self, trainer, pl_module, outputs, batch, batch_idx, dataloader_idx=0):
        if (trainer.current_epoch + 1) % self.log_every_n_epochs != 0:
            return
        self.log_samples("validation", trainer, pl_module, outputs, batch, batch_idx)

    @staticmethod
    def _decode(one_hot_like: torch.Tensor, classes: int) -> np.ndarray:
        """(B, Q, S) probabilities / one-hot -> (B, S) waveforms in [-1, 1]."""
        return mu_law_decode(one_hot_like.argmax(1).to(torch.int32), classes).cpu().numpy()

    def _decode_deemphasised(self, one_hot_like: torch.Tensor, classes: int) -> np.ndarray:
        """(B, Q, S) probabilities / one-hot -> (B, S) int16 PCM through the de-emphasis filter, whole clips."""
        return deemphasis_pcm16(one_hot_like.argmax(1).to(torch.int32).contiguous(), self.preemphasis,
                                classes).cpu().numpy()

    def log_samples(self, split, trainer, pl_module, outputs, batch, batch_idx):
        if getattr(trainer, "rank", 0) != 0:
            return
        root = self.out_dir or (Path(trainer.root) / "samples" if trainer.root is not None else None)
        if root is None:
            return
        audio, _, contexts, fps, _infos = batch
        # (a model with global classes was given each clip's own label; the row says which)
        labelled = bool(getattr(pl_module, "global_classes", None))
        Q = pl_module.config.model_config.input_channels
        decode, write = ((self._decode_deemphasised, write_pcm16) if self.preemphasis > 0.0
                         else (self._decode, write_wav))
        origin = decode(audio.to(outputs["output"].device), Q)
        pred = decode(outputs["output"], Q)
        gen = None
        if outputs.get("generated_output", None) is not None:
            gen = decode(outputs["generated_output"], Q)
        sweep = self.temperature_sweep if gen is not None else []
        if sweep and len(gen) != len(fps) * len(sweep):
            raise ValueError(f"generated_output holds {len(gen)} clips for {len(fps)} clips x {len(sweep)} temperatures")
        # (clip_length="native": a clip shorter than the prompt, the first RF samples, has nothing to prompt from --
        # it is left out and counted in the rows that are written)
        prompt_ok = outputs.get("prompt_ok", None) if gen is not None else None
        skipped_short = 0 if prompt_ok is None else sum(not ok for ok in prompt_ok)
        rows = []
        for i, fp in enumerate(fps):
            if prompt_ok is not None and not prompt_ok[i]:
                continue
            stem = f"epoch={trainer.current_epoch}-batch={batch_idx}-clip={i}"
            files = {"origin_audio": root / split / f"{stem}-origin.wav",
                     "pred_audio": root / split / f"{stem}-pred.wav"}
            write(files["origin_audio"], origin[i])
            write(files["pred_audio"], pred[i])
            for j, t in enumerate(sweep):
                swept = dict(files, gen_audio=root / split / f"{stem}-gen-T{t:g}.wav")
                write(swept["gen_audio"], gen[i * len(sweep) + j])
                rows.append({"split": split, "epoch": trainer.current_epoch, "batch_idx": batch_idx, "fp": fp,
                             **{k: str(v.relative_to(root)) for k, v in swept.items()}, "temperature": t})
            if sweep:
                continue
            if gen is not None:
                files["gen_audio"] = root / split / f"{stem}-gen.wav"
                write(files["gen_audio"], gen[i])
            rows.append({"split": split, "epoch": trainer.current_epoch, "batch_idx": batch_idx, "fp": fp,
                         **{k: str(v.relative_to(root)) for k, v in files.items()}})
        scores = outputs.get("sample_scores", None) if gen is not None else None
        if scores is not None:  # (--score_samples 1; rows are clip-major, len(sweep) or one per clip, as gen is)
            bits = scores["bits_per_sample"].cpu().tolist()
            source = scores["source_bits_per_sample"].cpu().tolist()
            # (--use_mel 1: the log-mel distance of each generated row from its source clip; absent otherwise)
            mel = {k: scores[k].cpu().tolist() for k in ("mel_distance_db", "mel_l1") if k in scores}
            # (--score_pitch 1: the pitch figures of the same pairs; a figure whose denominator is 0 is written as null)
            mel.update({k: [v if v == v else None for v in scores[k].cpu().tolist()]
                        for k in ("f0_rmse_cents", "vuv_error_rate", "gross_pitch_error_rate") if k in scores})
            per_clip = max(len(sweep), 1)
            kept = [i for i in range(len(fps)) if prompt_ok is None or prompt_ok[i]]
            for k, r in enumerate(rows):  # (the scores cover every clip of the batch; the rows only the kept ones)
                clip = kept[k // per_clip]
                r["bits_per_sample"] = bits[clip * per_clip + k % per_clip]
                r["source_bits_per_sample"] = source[clip]
                for name, values in mel.items():
                    r[name] = values[clip * per_clip + k % per_clip]
        if gen is not None and self.guidance != 1.0:  # (as a sweep's rows carry their temperature)
            for r in rows:
                r["guidance"] = self.guidance
        if self.preemphasis > 0.0:
            for r in rows:
                r["preemphasis"] = self.preemphasis
        if gen is not None and getattr(pl_module, "use_mel", False):
            # (each clip was generated under its SOURCE clip's log-mel frames: copy-synthesis)
            for r in rows:
                r["conditioning"] = "mel"
        if prompt_ok is not None:
            for r in rows:
                r["skipped_short"] = skipped_short
        if labelled:
            where = {str(fp): str(c) for fp, c in zip(fps, contexts)}
            for r in rows:
                r["context"] = where[str(r["fp"])]
        with open(root / "index.jsonl", "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
