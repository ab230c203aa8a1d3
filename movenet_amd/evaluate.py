"""Checkpoint + folder of WAVs -> objective figures, one JSON line per file.

    python -m movenet_amd.evaluate --checkpoint run/checkpoints/last.ckpt --wavs clips/ [--ema 1] [--synthesize 1] \\
        [--batch 16] [--temperature 1 --top_k 0 --top_p 1 --sampling model --seed 0] [--out report.jsonl]

Every ``*.wav`` of the folder goes through the loader's GPU front end as ``synthesize --from_wavs`` sends it (the whole
file, resampled by rate, under the checkpoint's pre-emphasis) and is scored teacher-forced as ONE row of
``WaveNet.score`` over its own length: ``bits_per_sample`` and ``accuracy`` of the file under the model, with its own
log-mel frames as conditioning where the checkpoint was trained with ``--use_mel 1``.  A file that resamples to more
than ``MAX_ROW_SAMPLES`` samples is refused (no tiling).

``--synthesize 1`` (a ``--use_mel 1`` checkpoint only) also regenerates each file from its own first RF samples under
its own frames -- ``generate()`` with the sampling flags of ``synthesize``; batch k draws on ``--seed`` + k -- and adds
what compares the copy with the source: ``mel_distance_db``, ``mel_l1`` and ``frames`` (``WaveNet.spectral_distance``:
the frames past the prompt and inside the file), and ``generated_bits_per_sample``, the copy's own likelihood.

``--pitch 1`` (with ``--synthesize 1``; ``--pitch_fmin 60 --pitch_fmax 500 --pitch_threshold 0.15``) also tracks the
pitch of the copy and of the source (``WaveNet.pitch_distance``) and adds ``f0_rmse_cents``,
``voiced_frames``, ``vuv_error_rate`` (frames voiced in exactly one of the two, over the frames compared) and
``gross_pitch_error_rate`` (voiced frames whose periods lie more than 20 % apart, over ``voiced_frames``), each null
where its denominator is 0.

The last line is the summary: ``{"files": n, "bits_per_sample": mean weighted by scored positions,
"mel_distance_db": mean weighted by frames (null without --synthesize)}`` and, with ``--pitch 1``, ``f0_rmse_cents``
(the root of the mean squared error weighted by ``voiced_frames``) and the two rates pooled over their denominators.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

from .callbacks import SAMPLE_RATE
from .synthesize import apply_settings, load_model, wav_batch, wav_indices

# The longest row one scoring pass takes in every precision (README, "Row length decides some forms": the bf16 layer
# kernels refuse rows above 2^21 columns); about 131 s at 16 kHz.
MAX_ROW_SAMPLES = 1 << 21


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m movenet_amd.evaluate", description=__doc__.split("\n\n")[0])
    a = p.add_argument
    a("--checkpoint", type=str, required=True)
    a("--wavs", type=str, required=True, help="every *.wav of this folder is evaluated")
    a("--ema", type=int, default=0, help="1: the averaged weights of a run with --ema_decay")
    # the five model flags: default, the checkpoint's hyper_parameters record; without one 256 / 64 / 64 / 10 / 3
    a("--input_channels", type=int, default=None)
    a("--residual_channels", type=int, default=None)
    a("--skip_channels", type=int, default=None)
    a("--layer_size", type=int, default=None)
    a("--stack_size", type=int, default=None)
    a("--synthesize", type=int, default=0, help="1: also copy-synthesise each file and compare (mel checkpoint)")
    a("--pitch", type=int, default=0, help="1: with --synthesize 1, also compare the pitch tracks of copy and source")
    a("--pitch_fmin", type=float, default=60.0)
    a("--pitch_fmax", type=float, default=500.0)
    a("--pitch_threshold", type=float, default=0.15)
    a("--label", type=str, default=None, help="one of the checkpoint's class names")
    a("--out", type=str, default=None, help="also write the lines to this file")
    a("--batch", type=int, default=16)
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
    return p


def weighted_mean(values, weights):
    """sum(v w) / sum(w) over the pairs with w > 0, or None when there are none."""
    pairs = [(float(v), int(w)) for v, w in zip(values, weights) if w > 0]
    total = sum(w for _, w in pairs)
    return sum(v * w for v, w in pairs) / total if total else None


def evaluate_batch(model, rec, paths, device, args, labels, seed, pitch_counts=None) -> list:
    """The records of one batch of files (dicts, in the order of ``paths``).  ``pitch_counts`` (a list, with
    ``--pitch 1``) gains each record's (vuv errors, gross errors, frames compared) for the summary's pooled rates."""
    rate = SAMPLE_RATE if rec is None else int(rec["audio_rate"])
    if rec is None:
        idx, lengths = wav_indices(model, rate, paths, device, MAX_ROW_SAMPLES)
        feats = None
    else:
        idx, lengths, feats = wav_batch(model, rec, paths, device, MAX_ROW_SAMPLES)
    rf = model.receptive_fields
    if int(idx.shape[1]) <= rf:
        raise ValueError(f"no file of {paths} is longer than the model's receptive field of {rf} samples")
    mel = {} if feats is None else {"local_features": feats}
    audio = model._one_hot_of(idx.contiguous(), torch.float32)
    res = model.score(audio, None, labels, lengths=lengths, **mel)
    bits, acc, pos = (t.cpu().tolist() for t in (res.bits_per_sample, res.accuracy, res.positions))
    records = [{"path": str(p), "samples": int(n), "seconds": int(n) / rate,
                "bits_per_sample": b if k > 0 else None, "accuracy": a if k > 0 else None, "positions": int(k)}
               for p, n, b, a, k in zip(paths, lengths, bits, acc, pos)]
    if args.synthesize:
        apply_settings(model, args, seed)
        model.generate_local_features = feats
        gen = model.generate(audio[:, :, :rf], None, labels, n_samples=int(idx.shape[1]),
                             temperature=args.temperature)
        dist = model.spectral_distance(gen, idx, lengths=lengths)
        own = model.score(gen, None, labels, lengths=lengths, **mel).bits_per_sample.cpu().tolist()
        for r, d, l1, f, g in zip(records, dist.lsd_db.cpu().tolist(), dist.l1.cpu().tolist(),
                                  dist.frames.cpu().tolist(), own):
            r.update(mel_distance_db=d, mel_l1=l1, frames=int(f),
                     generated_bits_per_sample=g if r["positions"] > 0 else None)
        if getattr(args, "pitch", 0):
            pd = model.pitch_distance(gen, idx, lengths=lengths, f_min=args.pitch_fmin, f_max=args.pitch_fmax,
                                      threshold=args.pitch_threshold)
            for r, e, both, vuv, gross, f in zip(records, *(t.cpu().tolist() for t in pd)):
                r.update(f0_rmse_cents=e if both > 0 else None, voiced_frames=int(both),
                         vuv_error_rate=vuv / f if f > 0 else None,
                         gross_pitch_error_rate=gross / both if both > 0 else None)
                if pitch_counts is not None:
                    pitch_counts.append((int(vuv), int(gross), int(f)))
    return records


def pitch_summary(records, pitch_counts) -> dict:
    """The pooled pitch figures of the summary line: the root of the mean squared error in cents weighted by
    ``voiced_frames``, and the two rates as summed numerators over summed denominators (None where those are 0).
    ``pitch_counts``: each record's (vuv errors, gross errors, frames compared), as ``evaluate_batch`` collects them."""
    both = sum(r["voiced_frames"] for r in records)
    vuv, gross, frames = (sum(c[i] for c in pitch_counts) for i in range(3))
    square = sum((r["f0_rmse_cents"] or 0.0) ** 2 * r["voiced_frames"] for r in records)
    return {"f0_rmse_cents": (square / both) ** 0.5 if both else None,
            "vuv_error_rate": vuv / frames if frames else None,
            "gross_pitch_error_rate": gross / both if both else None}


def main(argv=None) -> int:
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.batch < 1:
        parser.error("--batch must be at least 1")
    if args.pitch and not args.synthesize:
        parser.error("--pitch 1 needs --synthesize 1: the pitch of a copy is compared with its source's")
    model, rec, names = load_model(args, parser.error)
    if args.synthesize and rec is None:
        parser.error(f"--synthesize 1 needs a checkpoint trained with --use_mel 1: {args.checkpoint} has no "
                     "local_conditioning record")
    label = None
    if names:
        if args.label is None or args.label not in names:
            parser.error(f"this checkpoint is labelled: --label must be one of {names}")
        label = names.index(args.label)
    elif args.label is not None:
        parser.error(f"--label given, but {args.checkpoint} records no global_classes")
    files = sorted(str(p) for p in Path(args.wavs).glob("*.wav"))
    if not files:
        parser.error(f"no *.wav in {args.wavs}")
    device = torch.device(args.device)
    model = model.to(device).eval()
    sink = open(args.out, "w") if args.out else None
    records, pitch_counts = [], []

    def emit(record):
        line = json.dumps(record)
        print(line, flush=True)
        if sink is not None:
            sink.write(line + "\n")
    try:
        for k, b0 in enumerate(range(0, len(files), args.batch)):
            paths = files[b0:b0 + args.batch]
            labels = None if label is None else torch.full((len(paths),), label, dtype=torch.int64)
            try:
                batch = evaluate_batch(model, rec, paths, device, args, labels,
                                       None if args.seed is None else args.seed + k, pitch_counts)
            except ValueError as e:
                parser.error(str(e))
            for r in batch:
                emit(r)
            records += batch
        emit({"files": len(records),
              "bits_per_sample": weighted_mean([r["bits_per_sample"] or 0.0 for r in records],
                                               [r["positions"] for r in records]),
              "mel_distance_db": weighted_mean([r["mel_distance_db"] for r in records],
                                               [r["frames"] for r in records]) if args.synthesize else None,
              **(pitch_summary(records, pitch_counts) if args.pitch else {})})
    finally:
        if sink is not None:
            sink.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
