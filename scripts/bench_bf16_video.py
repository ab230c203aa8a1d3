"""Train-step time of video-conditioned training in bf16 at config 3 (8 x 32000, 32-frame clips, 10 x 3 layers, Q = 256,
C = K = 64; video encoder and up-sampler included), two modes in ONE process, alternating blocks of steps, medians:

    fp32_video     the conditioned step, fp32
    bf16_video     forward_precision = "bf16" with bf16_context = True (mvn_forward_bf16_ctx / mvn_backward_bf16_ctx)

    python scripts/bench_bf16_video.py [--blocks 5] [--steps 10] [--out profiles/bf16_video.json]

Writes one JSON: the two medians and their ratio.  Per-launch times of the layer kernels come from a
profiler's kernel trace of this script, in a run of its own (--out then names a file of that run: the timings under a
profiler are not the ones to quote).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import movenet_amd.wavenet as W  # noqa: E402
from movenet_amd.utils.weights import make_state_dict, one_hot, synthetic_indices  # noqa: E402

MODES = ("fp32_video", "bf16_video")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--clip_frames", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_video.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    cfg = dict(layer_size=10, stack_size=3, input_channels=256, residual_channels=64, skip_channels=64)
    # (the reference fixes the clip length through module constants: 32-frame clips <-> 32000 samples)
    W.MAX_VIDEO_FRAMES, W.MAX_AUDIO_FRAMES = a.clip_frames, 1000 * a.clip_frames
    t_len = 1000 * a.clip_frames
    model = W.WaveNet(**cfg)
    model.load_state_dict(make_state_dict(**cfg, seed=0), strict=False)
    model.to(dev).train()
    model.bf16_context = True
    x = one_hot(synthetic_indices(a.batch, t_len, 256, 1234).to(dev), 256)
    target = x[:, :, model.receptive_fields:].argmax(1)
    video = torch.from_numpy(np.random.default_rng(4321).random((a.batch, a.clip_frames, 64, 64, 1),
                                                                dtype=np.float32)).to(dev)

    def step(mode):
        model.forward_precision = mode.split("_")[0]
        model.zero_grad(set_to_none=True)
        loss, _, _ = model(x, video, return_loss=True, target=target)
        loss.backward()
        return loss

    losses = {}
    for mode in MODES:  # warm-up: code objects, allocator
        for _ in range(3):
            losses[mode] = float(step(mode))
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
        "what": "train step (forward + backward, no optimizer), config 3, ms (median of %d steps per mode, alternating "
                "blocks)" % (a.blocks * a.steps),
        "batch": a.batch, "frames": t_len, "median_ms": med,
        "min_ms": {mode: min(v) for mode, v in times.items()},
        "bf16_video_over_fp32_video": med["bf16_video"] / med["fp32_video"],
        "loss": losses,
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
