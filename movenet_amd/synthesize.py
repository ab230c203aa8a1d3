"""Checkpoint -> WAV files, written while they are being generated.

    python -m movenet_amd.synthesize --checkpoint run/checkpoints/last.ckpt \\
        --from_wavs clips/ --out synth/ --batch 16 --chunk 4000

The model's shape comes from the checkpoint's ``hyper_parameters`` record; ``--input_channels``, ``--residual_channels``,
``--skip_channels``, ``--layer_size`` and ``--stack_size`` are for files without one (defaults 256 / 64 / 64 / 10 / 3).

Two sources, exactly one per call:

* ``--from_wavs DIR``: copy-synthesis with a checkpoint trained under ``--use_mel 1``.  Every ``*.wav`` of DIR goes
  through the loader's GPU front end at the checkpoint's ``audio_rate`` (the whole file, resampled by rate), its class
  indices through ``ops.logmel`` with the checkpoint's mel settings, and the model regenerates the file under those
  frames from the file's own first RF samples.  The output has the (resampled) file's length and name.
* ``--seconds S --count N [--label NAME]``: N clips of S seconds from a prompt of silence; ``--label`` names one of the
  checkpoint's classes (required by a labelled checkpoint).

``WaveNet.generate_stream`` hands the PCM out chunk by chunk; each sequence has one ``wave`` writer that takes
``writeframesraw`` per chunk and fixes the header on close, so a closed file is byte for byte what
``callbacks.write_wav`` writes for the whole clip.  ``--context auto|whole|windowed`` (default auto) chooses how the
conditioning reaches the generators: ``windowed`` forms each chunk's columns in front of its launch, in memory that does
not grow with the clip; ``auto`` takes it where the whole context would exceed 1 GiB.  The audio is the same either way.  Batch k of a run draws on ``--seed`` + k.  One line per file goes to
stdout: path, samples, seconds of audio, wall seconds, seconds to the first generated chunk.

A checkpoint of a run with ``--preemphasis A`` records A: the model's PCM then comes out through the de-emphasis filter
and ``--from_wavs`` files go through the front end with that pre-emphasis, with no flag given.  ``--preemphasis``
overrides it for a checkpoint that records none; a value other than the recorded one is an error unless
``--force_preemphasis 1``.

``--pitch_shift SEMITONES`` (a checkpoint trained with ``--mel_f0 1``): the log-F0 channel of the ``--from_wavs``
features is moved by SEMITONES / 12 octaves; the log-mel and voicing channels stay the source's.  How far the output's
pitch follows depends on how much of the pitch the model learnt to read from that channel: the mel channels still carry
the source's harmonics.  On a checkpoint without the F0 record a non-zero value is an error.
"""
from __future__ import annotations

import argparse
import math
import os
import sys
import time
import wave
from pathlib import Path
from typing import List, Optional

import numpy as np
import torch

from .callbacks import SAMPLE_RATE


class IncrementalWav:
    """A mono 16-bit PCM WAV written in pieces: ``write`` appends int16 samples (``writeframesraw``), ``close`` fixes
    the header.  ``limit``: samples beyond it are dropped (a row of a batch that is longer than its own clip)."""

    def __init__(self, path, sample_rate: int, limit: Optional[int] = None):
        self.path = Path(path)
        self.path.parent.mkdir(parents=True, exist_ok=True)
        self.limit, self.written = limit, 0
        self._w = wave.open(str(self.path), "wb")
        self._w.setnchannels(1)
        self._w.setsampwidth(2)
        self._w.setframerate(int(sample_rate))

    @property
    def closed(self) -> bool:
        return self._w is None

    @property
    def full(self) -> bool:
        return self.limit is not None and self.written >= self.limit

    def write(self, pcm) -> int:
        """Append ``pcm`` (1-D int16); returns how many samples were taken."""
        pcm = np.asarray(pcm)
        if pcm.ndim != 1 or pcm.dtype != np.int16:
            raise ValueError(f"pcm must be 1-D int16, got {pcm.shape} {pcm.dtype}")
        if self.limit is not None:
            pcm = pcm[:max(self.limit - self.written, 0)]
        if pcm.size:
            self._w.writeframesraw(np.ascontiguousarray(pcm).astype("<i2", copy=False).tobytes())
            self.written += int(pcm.size)
        return int(pcm.size)

    def close(self) -> None:
        if self._w is not None:
            self._w.close()  # (patches the header's lengths to what was written)
            self._w = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def silence_class(classes: int) -> int:
    """The class mu-law gives 0.0 (what the front end pads with: csrc/audio.hip)."""
    return int(np.float32(classes - 1) / np.float32(2.0) + np.float32(0.5))


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m movenet_amd.synthesize", description=__doc__.split("\n\n")[0])
    a = p.add_argument
    a("--checkpoint", type=str, required=True)
    a("--ema", type=int, default=0, help="1: the averaged weights of a run with --ema_decay")
    # the five model flags: default, the checkpoint's hyper_parameters record; without one 256 / 64 / 64 / 10 / 3
    a("--input_channels", type=int, default=None)
    a("--residual_channels", type=int, default=None)
    a("--skip_channels", type=int, default=None)
    a("--layer_size", type=int, default=None)
    a("--stack_size", type=int, default=None)
    a("--from_wavs", type=str, default=None, help="copy-synthesis of every *.wav of this folder (mel checkpoint)")
    a("--seconds", type=float, default=None)
    a("--count", type=int, default=1)
    a("--label", type=str, default=None, help="one of the checkpoint's class names")
    a("--out", type=str, required=True)
    a("--batch", type=int, default=16)
    a("--chunk", type=int, default=4000)
    a("--temperature", type=float, default=1.0)
    a("--top_k", type=int, default=0)
    a("--top_p", type=float, default=1.0)
    a("--sampling", type=str, default="model", choices=["reference", "model"])
    a("--guidance", type=float, default=1.0)
    a("--seed", type=int, default=None)
    a("--precision", type=str, default="fp32", choices=["fp32", "fp16"])
    a("--device", type=str, default="cuda")
    a("--preemphasis", type=float, default=None, help="default: the checkpoint's record (0 without one)")
    a("--force_preemphasis", type=int, default=0, help="1: take --preemphasis against the checkpoint's record")
    a("--pitch_shift", type=float, default=0.0,
      help="semitones added to the F0 channel of a --mel_f0 1 checkpoint's features (--from_wavs)")
    a("--context", type=str, default="auto", choices=["auto", "whole", "windowed"],
      help="the generators' conditioning: built whole before the first step, or one window per chunk; auto: windowed "
           "where the whole context would take more than 1 GiB")
    return p


WHOLE_CONTEXT_LIMIT = 1 << 30  # bytes: beyond it --context auto takes the windowed path


def whole_context_bytes(rows: int, channels: int, n_total: int) -> int:
    """What the two whole-context tensors of a conditioned generator take: (rows, C, n_total) channel-major and its
    (rows, n_total, C) time-major copy, fp32."""
    return 2 * int(rows) * int(channels) * int(n_total) * 4


def context_mode(flag: str, conditioned: bool, rows: int, channels: int, n_total: int) -> str:
    """``--context``: "whole" / "windowed" as given; "auto": windowed where a conditioned model's two whole-context
    tensors would exceed 1 GiB, today's path otherwise (an unconditioned model builds no context: whole)."""
    if flag != "auto":
        return flag
    return "windowed" if conditioned and whole_context_bytes(rows, channels, n_total) > WHOLE_CONTEXT_LIMIT else "whole"


def load_model(args, fail):
    """The WaveNet of the model flags -- one not given (None) is filled in, in ``args``, from the checkpoint's
    ``hyper_parameters``, or without that record from the defaults 256 / 64 / 64 / 10 / 3 -- with the checkpoint's
    weights, on the CPU; ``local_conditioning`` and ``global_classes`` come from the checkpoint's records.  ``fail(message)`` is called (and must not return) where the
    flags and the state dict's shapes disagree, or ``--preemphasis`` and the checkpoint's record do.  The model's
    ``preemphasis`` is the record's, or the flag's where it may stand.  Returns (model, local record or None, class names)."""
    from .checkpoint import (CLI_MODEL_DEFAULTS, _local_record, _preemphasis_record, _read, _state_dict_of,
                             hyper_parameters_of, local_channels_of, local_window_of)
    from .wavenet import WaveNet
    obj = _read(args.checkpoint)
    # a model flag that was not given: the shape the checkpoint records (the trainer's hyper_parameters), else the default
    recorded = hyper_parameters_of(obj)
    for flag, default in CLI_MODEL_DEFAULTS.items():
        if getattr(args, flag, None) is None:
            setattr(args, flag, int(recorded.get(flag, default)))
    rec = _local_record(obj)
    names = list(obj.get("global_classes") or []) if isinstance(obj, dict) else []
    emph = _preemphasis_record(obj)
    if args.preemphasis is not None:
        if not 0.0 <= args.preemphasis < 1.0:
            fail(f"--preemphasis must lie in [0, 1), got {args.preemphasis}")
        # (a file without the record -- a run without the flag, or an older file -- says nothing: the flag stands)
        if emph > 0.0 and args.preemphasis != emph and not args.force_preemphasis:
            fail(f"--preemphasis {args.preemphasis} given, but {args.checkpoint} records preemphasis {emph}: the model "
                 "was trained on audio emphasised with that value (--force_preemphasis 1 to use the flag anyway)")
        emph = float(args.preemphasis)
    try:
        sd = _state_dict_of(obj, args.checkpoint, bool(args.ema))
    except ValueError as e:
        fail(str(e))
    # (the mel bins, and the two F0 channels of a --mel_f0 1 run behind them)
    local = {} if rec is None else {"local_channels": local_channels_of(rec), "local_hop": int(rec["local_hop"]),
                                    "local_window": local_window_of(rec)}  # (a record without the key: 0)
    model = WaveNet(args.layer_size, args.stack_size, args.input_channels, args.residual_channels, args.skip_channels,
                    global_classes=len(names), **local)
    want = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    have = {k: tuple(v.shape) for k, v in sd.items()}
    # (the decoder's tensors first: they name the flag at fault more plainly than the video encoder's)
    order = sorted(want, key=lambda k: k.startswith("video_"))
    wrong = [f"{k}: checkpoint {have[k]}, flags {want[k]}" for k in order if k in have and have[k] != want[k]]
    missing = [k for k in want if k not in have]
    extra = [k for k in have if k not in want]
    if wrong or missing or extra:
        parts = wrong[:3] + [f"missing from the checkpoint: {k}" for k in missing[:2]] + \
            [f"not in a model of these flags: {k}" for k in extra[:2]]
        fail(f"{args.checkpoint} does not fit --input_channels {args.input_channels} --residual_channels "
             f"{args.residual_channels} --skip_channels {args.skip_channels} --layer_size {args.layer_size} "
             f"--stack_size {args.stack_size} ({len(wrong)} shapes differ, {len(missing)} keys missing, {len(extra)} "
             "unexpected): " + "; ".join(parts))
    model.load_state_dict(sd, strict=True)
    model.preemphasis = emph
    if rec is not None:
        model.local_conditioning = rec
    return model, rec, names


def wav_indices(model, rate: int, paths: List[str], device, max_samples: Optional[int] = None):
    """One batch of files through the loader's GPU front end: (idx, lengths) -- ``idx`` (B, width) int32 class indices
    on the device, each file resampled as a whole to ``rate`` (``lengths[b]`` samples, silence behind them up to the
    batch's longest), under the model's pre-emphasis.  ``max_samples``: a file that resamples to more is a ValueError
    that names it and the limit, before anything is uploaded."""
    from .dataset import WavFolderLoader, _upload_pcm, read_wav_pcm16
    from .ops import audio_clip_var_descriptors, audio_frontend_var
    rate, device = int(rate), torch.device(device)
    clips = [read_wav_pcm16(p) for p in paths]
    lengths = [WavFolderLoader.native_plan(c[1], c[3], 1 << 30, rate)[1] for c in clips]
    for p, n in zip(paths, lengths):
        if max_samples is not None and n > max_samples:
            raise ValueError(f"{p} is {n} samples long at {rate} Hz: more than the {max_samples} samples of one row")
    width = max(lengths)
    Q = model.input_channels
    with torch.cuda.device(device):
        d_pcm, d_desc = _upload_pcm(device, [c[0] for c in clips], "clips_var", audio_clip_var_descriptors(
            [c[1] for c in clips], [c[2] for c in clips], lengths))
        # (the checkpoint's pre-emphasis: the indices, and with them the mel frames, are those training saw)
        emph = {"preemphasis": model.preemphasis} if model.preemphasis > 0.0 else {}
        idx = audio_frontend_var(d_pcm, d_desc, Q, width, normalize=True, **emph)
        if bool((idx < 0).any().item()):
            bad = [paths[b] for b in range(len(paths)) if bool((idx[b] < 0).any().item())]
            raise ValueError(f"the audio front end refused {bad[0]} (resampling ratio beyond what it takes)")
    return idx, lengths


def wav_batch(model, rec: dict, paths: List[str], device, max_samples: Optional[int] = None, shift=None):
    """The front end of copy-synthesis for one batch of files: (idx, lengths, feats) -- ``wav_indices`` at
    ``rec["audio_rate"]``, and ``feats``, the indices' local features by the checkpoint's record
    (``ops.local_features``: log-mel frames, with an ``"f0"`` entry the two F0 channels behind them, the log-F0 one
    moved by ``shift`` octaves)."""
    from .ops import local_features
    idx, lengths = wav_indices(model, int(rec["audio_rate"]), paths, torch.device(device), max_samples)
    feats = local_features(idx, model.input_channels, rec, shift=shift, lengths=lengths,
                           preemphasis=model.preemphasis)
    return idx, lengths, feats


def apply_settings(model, args, seed) -> None:
    model.generate_sampling = args.sampling
    model.generate_top_k, model.generate_top_p = args.top_k, args.top_p
    model.generate_precision = args.precision
    if args.guidance != 1.0:
        model.generate_guidance = float(args.guidance)
    model.generate_seed = seed


def stream_to_files(model, prompt_idx, n_total: int, lengths: List[int], paths: List[Path], sample_rate: int, args,
                    labels=None, feats=None, out=None) -> None:
    """One batch: ``generate_stream`` from ``prompt_idx`` (B, >= RF or fewer) into one incremental WAV per sequence,
    sequence b keeping its first ``lengths[b]`` samples; a line per file to ``out`` (default: stdout) when it closes."""
    out = sys.stdout if out is None else out
    began = time.perf_counter()
    writers = [IncrementalWav(p, sample_rate, limit=int(n)) for p, n in zip(paths, lengths)]
    first_chunk = None
    try:
        if feats is not None:
            model.generate_local_features = feats
        audio = model._one_hot_of(prompt_idx.contiguous(), torch.float32)
        rows = int(prompt_idx.shape[0]) * (2 if getattr(args, "guidance", 1.0) != 1.0 else 1)
        mode = context_mode(getattr(args, "context", "auto"), feats is not None or labels is not None, rows,
                            model.residual_channels, n_total)
        for t0, pcm in model.generate_stream(audio, None, labels, n_samples=n_total, temperature=args.temperature,
                                             chunk=args.chunk, context=mode):
            if t0 > 0 and first_chunk is None:
                first_chunk = time.perf_counter() - began
            for b, w in enumerate(writers):
                if w.closed:
                    continue
                w.write(pcm[b])
                if w.full:
                    _close(w, sample_rate, began, first_chunk, out)
    finally:
        for w in writers:
            if not w.closed:
                _close(w, sample_rate, began, first_chunk, out)


def _close(w: IncrementalWav, rate: int, began: float, first_chunk, out) -> None:
    w.close()
    first = "nan" if first_chunk is None else f"{first_chunk:.4f}"
    print(f"{w.path}\tsamples={w.written}\taudio_s={w.written / rate:.4f}\t"
          f"wall_s={time.perf_counter() - began:.4f}\tfirst_chunk_s={first}", file=out, flush=True)


def main(argv=None) -> int:
    parser = build_parser()
    args = parser.parse_args(argv)
    if (args.from_wavs is None) == (args.seconds is None):
        parser.error("give exactly one of --from_wavs DIR and --seconds S")
    if args.batch < 1 or args.chunk < 1 or args.count < 1:
        parser.error("--batch, --chunk and --count must be at least 1")
    if args.seconds is not None and not args.seconds > 0:
        parser.error("--seconds must be above 0")
    model, rec, names = load_model(args, parser.error)
    if args.from_wavs is not None and rec is None:
        parser.error(f"--from_wavs needs a checkpoint trained with --use_mel 1: {args.checkpoint} has no "
                     "local_conditioning record")
    if args.seconds is not None and rec is not None:
        parser.error(f"{args.checkpoint} was trained with --use_mel 1: it generates under log-mel frames, give "
                     "--from_wavs")
    if args.pitch_shift != 0.0:
        from .checkpoint import f0_record_of
        if not math.isfinite(args.pitch_shift):
            parser.error(f"--pitch_shift must be a finite number of semitones, got {args.pitch_shift}")
        if f0_record_of(rec) is None:
            parser.error(f"--pitch_shift {args.pitch_shift} needs a checkpoint trained with --mel_f0 1: "
                         f"{args.checkpoint} has no 'f0' entry in its local_conditioning record")
    label = None
    if names:
        if args.label is None or args.label not in names:
            parser.error(f"this checkpoint is labelled: --label must be one of {names}")
        label = names.index(args.label)
    elif args.label is not None:
        parser.error(f"--label given, but {args.checkpoint} records no global_classes")
    if args.from_wavs is not None:
        files = sorted(str(p) for p in Path(args.from_wavs).glob("*.wav"))
        if not files:
            parser.error(f"no *.wav in {args.from_wavs}")
    device = torch.device(args.device)
    model = model.to(device).eval()
    out_dir = Path(args.out)
    rf = model.receptive_fields

    def labels_for(n):
        return None if label is None else torch.full((n,), label, dtype=torch.int64)

    def seed_of(k):
        return None if args.seed is None else args.seed + k
    if args.from_wavs is not None:
        rate = int(rec["audio_rate"])
        for k, b0 in enumerate(range(0, len(files), args.batch)):
            paths = files[b0:b0 + args.batch]
            idx, lengths, feats = wav_batch(model, rec, paths, device, shift=args.pitch_shift / 12.0)
            apply_settings(model, args, seed_of(k))
            stream_to_files(model, idx[:, :rf], int(idx.shape[1]), lengths,
                            [out_dir / os.path.basename(p) for p in paths], rate, args, labels_for(len(paths)), feats)
    else:
        rate = SAMPLE_RATE
        n_total = max(int(round(args.seconds * rate)), 1)
        stem = "sample" if args.label is None else args.label
        for k, b0 in enumerate(range(0, args.count, args.batch)):
            n = min(args.batch, args.count - b0)
            prompt = torch.full((n, rf), silence_class(model.input_channels), dtype=torch.int32, device=device)
            apply_settings(model, args, seed_of(k))
            stream_to_files(model, prompt, n_total, [n_total] * n,
                            [out_dir / f"{stem}_{b0 + i:04d}.wav" for i in range(n)], rate, args, labels_for(n))
    return 0


if __name__ == "__main__":
    sys.exit(main())
