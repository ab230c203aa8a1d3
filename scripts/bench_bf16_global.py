"""Train-step time of labelled training in bf16 at config 2 (16 x 16000, 10 x 3 layers, Q = 256, C = K = 64), four modes in
ONE process, alternating blocks of steps, medians:

    fp32_audio     the audio-only step, fp32
    fp32_labels    labels on the fp32 fast path (backward choice (b): dfg tensor + row-sum kernel)
    bf16_audio     the audio-only step, forward_precision = "bf16"
    bf16_labels    labels under bf16, global_path = "bias" (backward choice (a): row sums inside the layer kernel)

    python scripts/bench_bf16_global.py [--blocks 5] [--steps 10] [--out profiles/bf16_global.json]

Writes one JSON: the four medians and the two overheads of the labels.  Per-launch times of the GLOBAL
kernel instantiations against the audio-only ones come from a profiler's kernel trace of this script, in a run of its own
(--out then names a file of that run: the timings under a profiler are not the ones to quote).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from movenet_amd.utils.weights import one_hot, synthetic_indices  # noqa: E402
from movenet_amd.wavenet import WaveNet  # noqa: E402

MODES = ("fp32_audio", "fp32_labels", "bf16_audio", "bf16_labels")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=16000)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_global.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    cfg = dict(layer_size=10, stack_size=3, input_channels=256, residual_channels=64, skip_channels=64)
    torch.manual_seed(0)
    plain = WaveNet(**cfg).to(dev).train()
    labelled = WaveNet(**cfg, global_classes=a.classes).to(dev).train()
    labelled.global_path = "bias"  # (fp32: the fast path, required; bf16: the labelled bf16 layer kernels)
    x = one_hot(synthetic_indices(a.batch, a.frames, 256, 1234), 256).to(dev)
    cls = torch.arange(a.batch) % a.classes  # (on the host, as the trainer passes them)

    def step(mode):
        precision, what = mode.split("_")
        m = plain if what == "audio" else labelled
        m.forward_precision = precision
        m.zero_grad(set_to_none=True)
        loss, _, _ = m(x, None, None if what == "audio" else cls, return_loss=True)
        loss.backward()

    for mode in MODES:  # warm-up: code objects, allocator
        for _ in range(3):
            step(mode)
    torch.cuda.synchronize()
    times = {mode: [] for mode in MODES}
    for _ in range(a.blocks):
        for mode in MODES:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
            ev[0].record()
            for i in range(a.steps):
                step(mode)
                ev[i + 1].record()
            torch.cuda.synchronize()
            times[mode] += [ev[i].elapsed_time(ev[i + 1]) for i in range(a.steps)]
    med = {mode: statistics.median(v) for mode, v in times.items()}
    result = {
        "what": "train step, config 2, ms (median of %d steps per mode, alternating blocks)" % (a.blocks * a.steps),
        "batch": a.batch, "frames": a.frames, "median_ms": med,
        "labels_over_audio_fp32": med["fp32_labels"] / med["fp32_audio"],
        "labels_over_audio_bf16": med["bf16_labels"] / med["bf16_audio"],
        "labels_cost_ms_fp32": med["fp32_labels"] - med["fp32_audio"],
        "labels_cost_ms_bf16": med["bf16_labels"] - med["bf16_audio"],
        "bf16_labels_over_fp32_labels": med["bf16_labels"] / med["fp32_labels"],
        "backward_choice": {"fp32": "b: WRITE_DFG layer kernel + row-sum kernel",
                            "bf16": "a: row sums inside the layer kernel + per-workgroup partials"},
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
