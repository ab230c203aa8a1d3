"""Train-step time of global conditioning at config 2 (16 x 16000, 10 x 3 layers, Q = 256, C = K = 64), three modes in
ONE process, alternating blocks of steps, medians:

    audio      the audio-only step
    fast       labels on the fast path (one bias vector per layer and sequence)
    context    labels through ``global_path = "context"`` (the conditioned kernels fed a constant context)

    python scripts/bench_global_conditioning.py [--blocks 5] [--steps 10] [--out profiles/global_conditioning.json]

Writes one JSON: the three medians, their ratios, and the bytes per layer the backward's choice (b) moves.
Per-kernel times come from a profiler's kernel trace of this script, in a run of its own.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=16000)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "global_conditioning.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    cfg = dict(layer_size=10, stack_size=3, input_channels=256, residual_channels=64, skip_channels=64)
    torch.manual_seed(0)
    plain = WaveNet(**cfg).to(dev).train()
    labelled = WaveNet(**cfg, global_classes=a.classes).to(dev).train()
    x = one_hot(synthetic_indices(a.batch, a.frames, 256, 1234), 256).to(dev)
    cls = torch.arange(a.batch) % a.classes  # (on the host, as the trainer passes them: their range check reads no device)

    def step(mode):
        m = plain if mode == "audio" else labelled
        if mode != "audio":
            m.global_path = "auto" if mode == "fast" else "context"
        m.zero_grad(set_to_none=True)
        loss, _, _ = m(x, None, None if mode == "audio" else cls, return_loss=True)
        loss.backward()

    modes = ("audio", "fast", "context")
    for mode in modes:  # warm-up: code objects, allocator
        for _ in range(3):
            step(mode)
    torch.cuda.synchronize()
    times = {mode: [] for mode in modes}
    for _ in range(a.blocks):
        for mode in modes:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
            ev[0].record()
            for i in range(a.steps):
                step(mode)
                ev[i + 1].record()
            torch.cuda.synchronize()
            times[mode] += [ev[i].elapsed_time(ev[i + 1]) for i in range(a.steps)]
    med = {mode: statistics.median(v) for mode, v in times.items()}
    tp = (a.frames + 63) // 64 * 64
    result = {
        "what": "train step, config 2, ms (median of %d steps per mode, alternating blocks)" % (a.blocks * a.steps),
        "batch": a.batch, "frames": a.frames, "median_ms": med,
        "fast_over_audio": med["fast"] / med["audio"], "context_over_audio": med["context"] / med["audio"],
        "fast_over_context": med["fast"] / med["context"],
        "backward_choice": "b: WRITE_DFG layer kernel + row-sum kernel",
        "dfg_bytes_per_layer": {"written": a.batch * 128 * tp * 4, "read": a.batch * 128 * a.frames * 4},
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
