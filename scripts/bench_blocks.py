"""The block path against the fused whole-model path at config 2's shape, in ONE process.

    python3 scripts/bench_blocks.py [--reps 20] [--warmup 3] [--out profiles/blocks.json]

Shape: batch 16, T = 16000, 10 x 3 layers, C = K = 64, Q = 256.  Two ways to the same logits, on the same weights:

    blocks   dense_conv(residual_conv_stack(causal_conv(x), None, S).sum(0))    (movenet_amd.modules, mvn_block_*)
    model    WaveNet.forward(x, output_unnormalized=False, remove_last=False)  (mvn_forward / mvn_backward)

each timed forward only (under no_grad) and forward + backward of ``(y * up).sum()``, the four legs interleaved, their
order rotating from repetition to repetition so that clock and thermal drift fall on all alike; medians of --reps
repetitions after --warmup of each, by stream events.  The block path has no pass mark -- it raised before it existed;
the ratio is what a caller pays for composing the blocks by hand.  Note the block path's memory: the stacked skip tensor
alone is 30 x 16 x 64 x 12929 floats = 1.6 GB, and with gradients every layer keeps its input, tanh and sigmoid."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CFG = dict(layer_size=10, stack_size=3, input_channels=256, residual_channels=64, skip_channels=64)
BATCH, T_LEN = 16, 16000


def _median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blocks.json"))
    a = ap.parse_args()
    import torch
    from movenet_amd import _native as N
    from movenet_amd.utils.weights import make_state_dict, one_hot, synthetic_indices
    from movenet_amd.wavenet import WaveNet
    t0 = time.perf_counter()
    dev = torch.device("cuda", 0)
    model = WaveNet(**CFG)
    model.load_state_dict(make_state_dict(**CFG, seed=0), strict=True)
    model = model.to(dev).train()
    Q = CFG["input_channels"]
    x = one_hot(synthetic_indices(BATCH, T_LEN, Q, 1234).to(dev), Q).to(torch.float32)
    S = model.compute_output_size(x)
    up = torch.randn(BATCH, Q, S, device=dev, generator=torch.Generator(device=dev).manual_seed(5))

    def blocks():
        return model.dense_conv(model.residual_conv_stack(model.causal_conv(x), None, S).sum(0))

    def whole():
        return model(x, output_unnormalized=False, remove_last=False)

    def fwd(path):
        with torch.no_grad():
            return path()

    def fwd_bwd(path):
        model.zero_grad(set_to_none=True)
        y = path()
        (y * up).sum().backward()
        return y

    legs = (("blocks_forward", lambda: fwd(blocks)), ("model_forward", lambda: fwd(whole)),
            ("blocks_forward_backward", lambda: fwd_bwd(blocks)), ("model_forward_backward", lambda: fwd_bwd(whole)))
    with torch.no_grad():  # (the form is that of the LAST block call: read it right behind the stack)
        sk = model.residual_conv_stack(model.causal_conv(x), None, S)
        form = N.lib().mvn_block_last_form()
        del sk
    y_b, y_m = fwd(blocks), fwd(whole)
    agree = float((y_b - y_m).abs().max() / y_m.abs().max())
    del y_b, y_m
    for name, leg in legs:
        for _ in range(a.warmup):
            leg()
    torch.cuda.synchronize(dev)
    times = {name: [] for name, _ in legs}
    for rep in range(a.reps):
        r = rep % len(legs)
        for name, leg in legs[r:] + legs[:r]:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            leg()
            ev[1].record()
            torch.cuda.synchronize(dev)
            times[name].append(ev[0].elapsed_time(ev[1]))
    med = {name: _median(v) for name, v in times.items()}
    res = {
        "workload": "config 2 shape: batch 16, T 16000, 10 x 3 layers, C = K = 64, Q = 256; logits of "
                    "dense_conv(stack(causal_conv(x), None, S).sum(0)) against WaveNet.forward on the same weights",
        "timing": f"four legs interleaved in one process, rotating order, median of {a.reps} repetitions after "
                  f"{a.warmup} warm-ups of each (stream events)",
        "skip_columns": S,
        "stacked_skip_tensor_GB": 30 * BATCH * 64 * S * 4 / 1e9,
        "block_form_of_the_stack": form,
        "max_abs_difference_over_max_abs": agree,
        "ms_median": med,
        "ms_min_max": {name: [min(v), max(v)] for name, v in times.items()},
        "ratio_blocks_over_model_forward": med["blocks_forward"] / med["model_forward"],
        "ratio_blocks_over_model_forward_backward": med["blocks_forward_backward"] / med["model_forward_backward"],
        "peak_memory_GB": torch.cuda.max_memory_allocated(dev) / 1e9,
        "device": torch.cuda.get_device_name(0),
        "ms": {name: [round(t, 3) for t in v] for name, v in times.items()},
    }
    res["wall_s"] = time.perf_counter() - t0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "ms"}))


if __name__ == "__main__":
    main()
