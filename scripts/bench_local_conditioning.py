"""Local conditioning on log-mel frames at config 2's shape (16 x 16000, 10 x 3 layers, Q = 256, C = K = 64; N = 1024,
hop 256, M = 80), ONE process, alternating blocks, medians:

    stream time of the front end (ops.logmel) and of the up-sampler, forward and backward (ops.upsample_features)
    the train step  audio    audio-only
                    label    a class label through global_path = "context" (the conditioned kernels, constant context)
                    mel      local_features = the batch's own log-mel frames, computed inside the step as the trainer does

    python scripts/bench_local_conditioning.py [--blocks 5] [--steps 10] [--out profiles/local_conditioning.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from movenet_amd import ops  # noqa: E402
from movenet_amd.utils.weights import one_hot, synthetic_indices  # noqa: E402
from movenet_amd.wavenet import WaveNet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=16000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_conditioning.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    n_fft, hop, n_mels = 1024, 256, 80
    cfg = dict(layer_size=10, stack_size=3, input_channels=256, residual_channels=64, skip_channels=64)
    torch.manual_seed(0)
    plain = WaveNet(**cfg).to(dev).train()
    labelled = WaveNet(**cfg, global_classes=8).to(dev).train()
    labelled.global_path = "context"
    local = WaveNet(**cfg, local_channels=n_mels, local_hop=hop).to(dev).train()
    idx = synthetic_indices(a.batch, a.frames, 256, 1234).to(dev)
    x = one_hot(idx.cpu(), 256).to(dev)
    cls = torch.arange(a.batch) % 8
    fbank = torch.from_numpy(ops.mel_filterbank(n_mels, n_fft, 16000.0)).to(device=dev, dtype=torch.float32)
    feats = ops.logmel(idx, 256, n_fft, hop, fbank)
    dctx = torch.randn(a.batch, 64, a.frames, device=dev)

    def train(mode):
        m = {"audio": plain, "label": labelled, "mel": local}[mode]
        m.zero_grad(set_to_none=True)
        if mode == "mel":
            with torch.no_grad():
                f = ops.logmel(x.argmax(1).to(torch.int32), 256, n_fft, hop, fbank)
            loss, _, _ = m(x, return_loss=True, local_features=f)
        else:
            loss, _, _ = m(x, None, cls if mode == "label" else None, return_loss=True)
        loss.backward()

    def frontend(_):
        ops.logmel(idx, 256, n_fft, hop, fbank)

    def up_forward(_):
        with torch.no_grad():
            ops.upsample_features(local, feats, a.frames)

    def up_both(_):
        local.zero_grad(set_to_none=True)
        ops.upsample_features(local, feats, a.frames).backward(dctx)

    cases = [("frontend", frontend, None), ("upsample_forward", up_forward, None),
             ("upsample_forward_backward", up_both, None), ("step_audio", train, "audio"), ("step_label", train, "label"),
             ("step_mel", train, "mel")]
    for _, fn, arg in cases:  # warm-up: code objects, allocator
        for _ in range(3):
            fn(arg)
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in cases}
    for _ in range(a.blocks):
        for name, fn, arg in cases:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
            ev[0].record()
            for i in range(a.steps):
                fn(arg)
                ev[i + 1].record()
            torch.cuda.synchronize()
            times[name] += [ev[i].elapsed_time(ev[i + 1]) for i in range(a.steps)]
    med = {name: statistics.median(v) for name, v in times.items()}
    result = {
        "what": "stream time between events, ms (median of %d per case, alternating blocks, one process)" % (a.blocks * a.steps),
        "batch": a.batch, "frames": a.frames, "n_fft": n_fft, "hop": hop, "n_mels": n_mels, "median_ms": med,
        "upsample_backward_ms": med["upsample_forward_backward"] - med["upsample_forward"],
        "mel_over_audio": med["step_mel"] / med["step_audio"], "mel_over_label": med["step_mel"] / med["step_label"],
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
