"""The windowed frame up-sampler, ONE process, alternating blocks, medians of stream time between events:

(a) mvn_upsample_features_win, forward and forward + backward, at taps 1, 5 and 9, against the existing call
    (mvn_upsample_features, the yardstick) and against replicate-pad + torch.nn.functional.conv1d + interpolation in
    torch (taps 5), at two shapes: config 2's (16, 80, 63 frames -> 64 channels, hop 256, T 16000) and a whole file
    (1, 80, 8192 frames, hop 256, T 2097152);
(b) the config-2 train step under --use_mel 1 (features computed inside the step, as the trainer does), local_window 0
    against 2.

    python scripts/bench_local_window.py [--blocks 5] [--steps 10] [--out profiles/local_window.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from movenet_amd import _native as N  # noqa: E402
from movenet_amd import ops  # noqa: E402
from movenet_amd.utils.weights import one_hot, synthetic_indices  # noqa: E402
from movenet_amd.wavenet import WaveNet  # noqa: E402

DEV = "cuda:0"
SHAPES = {"config2": (16, 80, 63, 64, 256, 16000), "whole_file": (1, 80, 8192, 64, 256, 8192 * 256)}


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def kernel_cases(name, shape):
    """(label, callable) pairs of measurement (a) at one shape; every buffer is allocated once, outside the timing."""
    B, M, Fr, C, hop, T = shape
    lib = N.lib()
    g = torch.Generator().manual_seed(1)
    mel = torch.randn(B, M, Fr, generator=g).to(DEV)
    bias = torch.randn(C, generator=g).to(DEV)
    dctx = torch.randn(B, C, T, generator=g).to(DEV)
    ctx = torch.empty(B, C, T, device=DEV)
    dmel = torch.empty(B, M, Fr, device=DEV)
    db = torch.zeros(C, device=DEV)
    n = int(lib.mvn_upsample_features_scratch_floats(B, C, Fr))
    scratch = torch.empty(n, device=DEV)
    cases = []

    def c_calls(taps, existing):
        w = (torch.randn(C, M, taps, generator=g) / (M * taps) ** 0.5).to(DEV)
        dw = torch.zeros_like(w)

        def forward():
            if existing:
                rc = lib.mvn_upsample_features(mel.data_ptr(), Fr, w.data_ptr(), bias.data_ptr(), B, M, Fr, C, hop, T,
                                               ctx.data_ptr(), T, scratch.data_ptr(), n, _stream())
            else:
                rc = lib.mvn_upsample_features_win(mel.data_ptr(), Fr, w.data_ptr(), bias.data_ptr(), B, M, Fr, C, taps,
                                                   hop, T, ctx.data_ptr(), T, scratch.data_ptr(), n, _stream())
            N.check(rc, "forward")

        def both():
            forward()
            if existing:
                rc = lib.mvn_upsample_features_backward(dctx.data_ptr(), T, mel.data_ptr(), Fr, w.data_ptr(), B, M, Fr, C,
                                                        hop, T, dw.data_ptr(), db.data_ptr(), dmel.data_ptr(), Fr,
                                                        scratch.data_ptr(), n, _stream())
            else:
                rc = lib.mvn_upsample_features_win_backward(dctx.data_ptr(), T, mel.data_ptr(), Fr, w.data_ptr(), B, M,
                                                            Fr, C, taps, hop, T, dw.data_ptr(), db.data_ptr(),
                                                            dmel.data_ptr(), Fr, scratch.data_ptr(), n, _stream())
            N.check(rc, "backward")
        return forward, both

    fwd, both = c_calls(1, True)
    cases += [(f"{name}/existing/forward", fwd), (f"{name}/existing/forward_backward", both)]
    for taps in (1, 5, 9):
        fwd, both = c_calls(taps, False)
        cases += [(f"{name}/win_taps{taps}/forward", fwd), (f"{name}/win_taps{taps}/forward_backward", both)]

    # torch: replicate padding, conv1d, the interpolation by indexing
    k = 2
    w_t = (torch.randn(C, M, 2 * k + 1, generator=g) / (M * 5) ** 0.5).to(DEV).requires_grad_(True)
    b_t = bias.clone().requires_grad_(True)
    mel_t = mel.clone().requires_grad_(True)
    t = torch.arange(T, device=DEV)
    j = t // hop
    j1 = torch.clamp(j + 1, max=Fr - 1)
    a = ((t % hop).float() / hop)[None, None, :]

    def torch_forward():
        proj = F.conv1d(F.pad(mel_t, (k, k), mode="replicate"), w_t, b_t)
        return (1.0 - a) * proj[:, :, j] + a * proj[:, :, j1]

    def torch_fwd_only():
        with torch.no_grad():
            torch_forward()

    def torch_both():
        for v in (w_t, b_t, mel_t):
            v.grad = None
        torch_forward().backward(dctx)
    cases += [(f"{name}/torch_taps5/forward", torch_fwd_only), (f"{name}/torch_taps5/forward_backward", torch_both)]
    return cases


def step_cases(batch, frames):
    """Measurement (b): the config-2 train step with the batch's own log-mel frames, local_window 0 and 2."""
    n_fft, hop, n_mels = 1024, 256, 80
    cfg = dict(layer_size=10, stack_size=3, input_channels=256, residual_channels=64, skip_channels=64)
    torch.manual_seed(0)
    models = {k: WaveNet(**cfg, local_channels=n_mels, local_hop=hop, local_window=k).to(DEV).train() for k in (0, 2)}
    idx = synthetic_indices(batch, frames, 256, 1234).to(DEV)
    x = one_hot(idx.cpu(), 256).to(DEV)
    fbank = torch.from_numpy(ops.mel_filterbank(n_mels, n_fft, 16000.0)).to(device=DEV, dtype=torch.float32)

    def step(k):
        def run():
            m = models[k]
            m.zero_grad(set_to_none=True)
            with torch.no_grad():
                f = ops.logmel(x.argmax(1).to(torch.int32), 256, n_fft, hop, fbank)
            loss, _, _ = m(x, return_loss=True, local_features=f)
            loss.backward()
        return run
    return [("step/local_window0", step(0)), ("step/local_window2", step(2))]


def measure(cases, blocks, steps):
    for _, fn in cases:  # warm-up: code objects, allocator, torch's algorithm choice
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in cases}
    for _ in range(blocks):
        for name, fn in cases:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
            ev[0].record()
            for i in range(steps):
                fn()
                ev[i + 1].record()
            torch.cuda.synchronize()
            times[name] += [ev[i].elapsed_time(ev[i + 1]) for i in range(steps)]
    return {name: statistics.median(v) for name, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_window.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_local_window.py measures on the GPU: none found")
    med = {}
    for name, shape in SHAPES.items():
        med.update(measure(kernel_cases(name, shape), a.blocks, a.steps))
        torch.cuda.empty_cache()
    med.update(measure(step_cases(16, 16000), a.blocks, a.steps))
    backward = {k[:-len("/forward_backward")] + "/backward": v - med[k[:-len("_backward")]]
                for k, v in med.items() if k.endswith("/forward_backward")}
    result = {
        "what": "stream time between events, ms (median of %d per case, alternating blocks, one process); backward = "
                "forward_backward - forward" % (a.blocks * a.steps),
        "shapes": {k: dict(zip(("batch", "n_mels", "frames", "channels", "hop", "n_samples"), v)) for k, v in SHAPES.items()},
        "median_ms": med, "backward_ms": backward,
        "step_window2_over_window0": med["step/local_window2"] / med["step/local_window0"],
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
