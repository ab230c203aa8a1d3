"""fp32 against bf16 training (WaveNet.forward_precision = "bf16") on the config-2 train step, in ONE process.

    python3 scripts/bench_bf16_train.py [--blocks 6] [--steps 5] [--out profiles/bf16_train.json]
    rocprofv3 --kernel-trace --stats -d out -- python3 scripts/bench_bf16_train.py --blocks 2 --out out/bf16_train_rp.json
    python3 scripts/bench_bf16_train.py --kernel-stats out/.../kernel_stats.csv   (no GPU: adds the layer kernels'
        us and GB/s to --out from a kernel-stats file of the run above; where rocprofv3 writes a results database
        instead, `rocpd2summary -i out/run_results.db -d DIR --format csv` makes DIR/kernels_summary.csv of it)

The step is bench.py's train leg (config 2: 30 layers, Q = 256, C = K = 64, 16 clips x 16000 samples, the trainer's
fused loss, backward, FlatAdamW).  The two modes alternate in blocks of --steps steps after a warm-up of each, so that
clock and thermal drift fall on both alike; each step is timed by stream events, each mode reports the median of all
its steps, and the ratio bf16 / fp32 is of the two medians."""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CFG = dict(layer_size=10, stack_size=3, input_channels=256, residual_channels=64, skip_channels=64)
BATCH, T_LEN = 16, 16000
KERNELS = {  # the layer kernels of each mode, as rocprofv3 names them
    "fp32_forward": "fused_layer64s_bf3_kernel", "fp32_backward": "bwd_layer64_kernel<false>",
    "bf16_forward": "fused_layer64s_bf16_kernel", "bf16_backward": "bwd_layer64_bf16_kernel",
}


def layer_bytes(cfg=CFG, batch=BATCH, t_len=T_LEN):
    """Mean HBM bytes per layer launch that the forward and the backward layer kernel must move (fp32 tensors, each
    read or written once; bench.train_bytes_per_step's per-layer terms):
      forward   x(t), x(t - d) read; x', tanh, sigmoid written (no x' for the last layer); skip sum read + written
                where t >= RF - 1 (written only by the first layer)
      backward  A', P0 of the layer above (not for the last layer), dskip (t >= RF - 1), tanh, sigmoid, x(t), x(t - d)
                read; A', P0 written"""
    C = cfg["residual_channels"]
    ds = [2 ** i for _ in range(cfg["stack_size"]) for i in range(cfg["layer_size"])]
    L, rf = len(ds), sum(ds) + cfg["stack_size"]
    S = t_len - rf + 1
    fwd = bwd = 0
    a = 0
    for li, d in enumerate(ds):
        a += d
        n, ns = t_len - a, min(t_len - a, S)
        last, first = li == L - 1, li == 0
        fwd += n * (2 * C + (0 if last else C) + 2 * C) + ns * (C + (0 if first else C))
        bwd += n * ((0 if last else 2 * C) + 4 * C + 2 * C) + ns * C
    return {"forward": 4.0 * batch * fwd / L, "backward": 4.0 * batch * bwd / L}


def run(blocks: int, steps: int, warmup: int) -> dict:
    import torch
    from movenet_amd import _native as N
    from movenet_amd.optim import FlatAdamW, order_like_backward
    from movenet_amd.utils.weights import make_state_dict, one_hot, synthetic_indices
    from movenet_amd.wavenet import WaveNet
    dev = torch.device("cuda", 0)
    model = WaveNet(**CFG)
    model.load_state_dict(make_state_dict(**CFG, seed=0), strict=True)
    model.to(dev).train()
    opt = FlatAdamW(order_like_backward(model, with_context=False), lr=1e-4)
    Q, rf = CFG["input_channels"], model.receptive_fields
    audio = one_hot(synthetic_indices(BATCH, T_LEN, Q, 1234).to(dev), Q)
    target = audio[:, :, rf:].argmax(1)

    def step():
        opt.zero_grad(set_to_none=True)
        loss, _, _ = model(audio, None, return_loss=True, target=target)
        loss.backward()
        opt.step()
        return loss

    modes = {"fp32": "fp32", "bf16": "bf16"}
    times = {m: [] for m in modes}
    losses = {m: [] for m in modes}
    forms = {}
    for m, prec in modes.items():  # warm-up of each mode (allocator, LDS attributes, weight images)
        model.forward_precision = prec
        for _ in range(warmup):
            step()
        forms[m] = N.lib().mvn_last_backward_form()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for blk in range(blocks):
        for m in (("fp32", "bf16") if blk % 2 == 0 else ("bf16", "fp32")):
            model.forward_precision = modes[m]
            marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
            marks[0].record()
            for i in range(steps):
                loss = step()
                marks[i + 1].record()
                losses[m].append(loss.detach())  # (the loss itself would keep its graph and buffers alive)
            torch.cuda.synchronize(dev)
            times[m] += [marks[i].elapsed_time(marks[i + 1]) for i in range(steps)]
    wall = time.perf_counter() - t0
    med = {m: sorted(v)[len(v) // 2] for m, v in times.items()}
    tokens = BATCH * (T_LEN - rf)
    return {
        "workload": "config 2 train step (bench.py train leg): 30 layers, Q=256, C=K=64, 16 x 16000, fused loss, "
                    "backward, FlatAdamW",
        "timing": f"{blocks} alternating blocks of {steps} steps per mode after {warmup} warm-ups each, one process; "
                  "median of each mode's steps (stream events)",
        "fp32_ms_median": med["fp32"], "bf16_ms_median": med["bf16"], "ratio_bf16_over_fp32": med["bf16"] / med["fp32"],
        "fp32_tokens_per_s": tokens / (med["fp32"] * 1e-3), "bf16_tokens_per_s": tokens / (med["bf16"] * 1e-3),
        "fp32_ms_steps": [round(x, 3) for x in times["fp32"]], "bf16_ms_steps": [round(x, 3) for x in times["bf16"]],
        "backward_form": {m: f for m, f in forms.items()},
        "last_loss": {m: float(v[-1]) for m, v in losses.items()},
        "wall_s": wall, "device": torch.cuda.get_device_name(dev),
        "layer_bytes": layer_bytes(),
    }


def kernel_rates(stats_csv: str) -> dict:
    """us per launch and HBM GB/s (layer_bytes over the mean duration) of the four layer kernels."""
    nb = layer_bytes()
    rows = {}
    with open(stats_csv) as f:
        for r in csv.DictReader(f):
            rows[r["Name"]] = r
    out = {}
    for key, name in KERNELS.items():
        hit = [r for n, r in rows.items() if name in n]
        if not hit:
            continue
        r = hit[0]
        us = float(r.get("AverageNs") or r["Average (Nsec)"]) * 1e-3  # (--stats CSV, or rocpd2summary's of the .db)
        b = nb[key.split("_")[1]]
        out[key] = {"kernel": r["Name"], "calls": int(r["Calls"]), "avg_us": us, "bytes": b, "GB_per_s": b / (us * 1e3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_train.json"))
    ap.add_argument("--kernel-stats", default=None, help="add the layer kernels' rates from this file to --out")
    a = ap.parse_args()
    if a.kernel_stats:
        with open(a.out) as f:
            res = json.load(f)
        res["kernels"] = kernel_rates(a.kernel_stats)
    else:
        res = run(a.blocks, a.steps, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if not k.endswith("_steps")}))


if __name__ == "__main__":
    main()
