"""The config-2 train step with the weights' moving average (FlatAdamW(ema_decay=...)) off and on, in ONE process.

    python3 scripts/bench_ema.py [--blocks 6] [--steps 5] [--out profiles/ema.json] [--bench-lines FILE]

The step is bench.py's train leg (config 2: 30 layers, Q = 256, C = K = 64, 16 clips x 16000 samples, the trainer's
fused loss, backward, FlatAdamW).  Three legs alternate in blocks of --steps steps after a warm-up of each, their order
rotating from block to block so that clock and thermal drift fall on all alike: the average off, on, and off AGAIN -- the
two "off" legs differ by nothing but their place in the rotation, so the gap between their medians is the run-to-run
spread the "on" median is read against.  Each step is timed by stream events.  Two models from the same weights, one per
optimizer: a model's parameters are views into its optimizer's buffer.

The optimizer launch alone (mvn_adamw_step against mvn_adamw_ema_step on the step's flat span): --kernel-burst
back-to-back launches between ONE pair of HIP events, divided by their number, the two entry points alternating.  That
is the stream's time per launch in a burst -- the gap between consecutive launches included -- not a profiler's kernel
time, and the GB/s derived from it is a lower bound on what the kernel itself streams.

--bench-lines FILE: a file of JSON lines {"tree": "parent" | "change", "run": k, "line": <bench.py's result line>},
written by alternating runs of ``bench.py --gpus 1 --full --no-cpu-baseline --no-extras`` on this tree and on its
parent; their headline and train legs are summarised under "bench_py" in the same output file."""
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
EMA_DECAY = 0.999
LEGS = (("off", "off"), ("on", "on"), ("off_again", "off"))


def _median(v):
    return sorted(v)[len(v) // 2]


def train_steps(blocks: int, steps: int, warmup: int) -> dict:
    import torch
    from movenet_amd.optim import FlatAdamW, order_like_backward
    from movenet_amd.utils.weights import make_state_dict, one_hot, synthetic_indices
    from movenet_amd.wavenet import WaveNet
    dev = torch.device("cuda", 0)
    models, opts = {}, {}
    for name, decay in (("off", 0.0), ("on", EMA_DECAY)):
        model = WaveNet(**CFG)
        model.load_state_dict(make_state_dict(**CFG, seed=0), strict=True)
        models[name] = model.to(dev).train()
        opts[name] = FlatAdamW(order_like_backward(model, with_context=False), lr=1e-4, ema_decay=decay)
    Q, rf = CFG["input_channels"], models["off"].receptive_fields
    audio = one_hot(synthetic_indices(BATCH, T_LEN, Q, 1234).to(dev), Q)
    target = audio[:, :, rf:].argmax(1)

    def step(name):
        model, opt = models[name], opts[name]
        opt.zero_grad(set_to_none=True)
        loss, _, _ = model(audio, None, return_loss=True, target=target)
        loss.backward()
        opt.step()
        return loss

    times = {leg: [] for leg, _ in LEGS}
    last = {}
    for name in ("off", "on"):  # warm-up of each (allocator, LDS attributes, code objects)
        for _ in range(warmup):
            step(name)
    torch.cuda.synchronize(dev)
    for blk in range(blocks):
        r = blk % len(LEGS)
        for leg, name in LEGS[r:] + LEGS[:r]:
            marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
            marks[0].record()
            for i in range(steps):
                loss = step(name)
                marks[i + 1].record()
            last[leg] = loss.detach()
            torch.cuda.synchronize(dev)
            times[leg] += [marks[i].elapsed_time(marks[i + 1]) for i in range(steps)]
    med = {leg: _median(v) for leg, v in times.items()}
    return {
        "ema_decay": EMA_DECAY,
        "parameters": opts["on"].flat.numel(),
        "optimizer_launches_per_step": {n: o.last_launches for n, o in opts.items()},
        "step_ms_median": med,
        "step_ms_off_spread": abs(med["off"] - med["off_again"]),
        "step_ratio_on_over_off": med["on"] / min(med["off"], med["off_again"]),
        "on_within_spread_or_below": med["on"] <= max(med["off"], med["off_again"]),
        "step_ms": {leg: [round(x, 3) for x in v] for leg, v in times.items()},
        "last_loss": {leg: float(v) for leg, v in last.items()},
        "tokens_per_step": BATCH * (T_LEN - rf),
    }


def optimizer_launch(n: int, reps: int, warmup: int, burst: int) -> dict:
    """`burst` back-to-back launches over n elements between one pair of HIP events, per entry point, alternating:
    stream time per launch of a burst (launch gaps included), not kernel time from a profiler."""
    import ctypes
    import torch
    from movenet_amd import _native as N
    lib = N.lib()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(3)
    p, grad = torch.randn(n, generator=g, device=dev), torch.randn(n, generator=g, device=dev)
    m, v, e = torch.zeros_like(p), torch.zeros_like(p), p.clone()
    none = (ctypes.c_size_t * 1)(0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    hyper = (1e-4, 0.9, 0.999, 1e-8, 0.01)

    def plain(k):
        N.check(lib.mvn_adamw_step(p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), n, *hyper, k, 1, none,
                                   0, stream), "mvn_adamw_step")

    def with_ema(k):
        N.check(lib.mvn_adamw_ema_step(p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), e.data_ptr(), n,
                                       *hyper, k, 1, 1.0 - EMA_DECAY, none, 0, stream), "mvn_adamw_ema_step")

    calls = {"mvn_adamw_step": plain, "mvn_adamw_ema_step": with_ema}
    us = {name: [] for name in calls}
    for i in range(warmup + reps):
        for name in (list(calls) if i % 2 == 0 else list(calls)[::-1]):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for k in range(burst):
                calls[name](i * burst + k + 1)
            ev[1].record()
            torch.cuda.synchronize(dev)
            if i >= warmup:
                us[name].append(1e3 * ev[0].elapsed_time(ev[1]) / burst)
    out = {"elements": n, "what": f"stream time per launch: {burst} back-to-back launches between one event pair, "
                                  f"median of {reps} bursts; launch gaps included, not a profiler's kernel time"}
    for name, words in (("mvn_adamw_step", 7), ("mvn_adamw_ema_step", 9)):  # p, g, m, v read; p, m, v written (+ ema both)
        t = _median(us[name])
        out[name] = {"us_per_launch": t, "GB_per_s_at_least": 4 * words * n / (t * 1e3)}
    return out


def bench_lines(path: str) -> dict:
    """Headline and train legs of the alternating bench.py runs: every run's values, and whether each of this tree's
    lies inside [min, max] of the parent's own repeats."""
    runs = [json.loads(l) for l in open(path) if l.strip()]
    pick = {"headline_samples_per_s": lambda d: d["value"],
            "train_step_ms": lambda d: d["train_step"]["ms_per_step"],
            "train_step_config3_ms": lambda d: d["train_step_config3"]["ms_per_step"]}
    out = {"order": [f'{r["tree"]}{r["run"]}' for r in runs], "command": "bench.py --gpus 1 --steps 3 --warmup 1 --full "
           "--no-cpu-baseline --no-extras"}
    for key, get in pick.items():
        vals = {tree: [] for tree in ("parent", "change")}
        for r in runs:
            try:
                vals[r["tree"]].append(get(r["line"]))
            except (KeyError, TypeError):
                pass
        if not vals["parent"] or not vals["change"]:
            continue
        lo, hi = min(vals["parent"]), max(vals["parent"])
        inside = [lo <= x <= hi for x in vals["change"]]
        out[key] = {**vals, "parent_spread": [lo, hi], "change_inside_parent_spread": inside,
                    "change_runs_outside": inside.count(False), "change_runs": len(inside),
                    "parent_median": _median(vals["parent"]), "change_median": _median(vals["change"])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--kernel-burst", type=int, default=100)
    ap.add_argument("--bench-lines", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema.json"))
    a = ap.parse_args()
    import torch
    t0 = time.perf_counter()
    steps = train_steps(a.blocks, a.steps, a.warmup)
    res = {
        "workload": "config 2 train step (bench.py train leg): 30 layers, Q=256, C=K=64, 16 x 16000, fused loss, "
                    "backward, FlatAdamW with ema_decay 0 (off) and 0.999 (on)",
        "timing": f"{a.blocks} blocks of {a.steps} steps per leg (off, on, off again; rotating order) after {a.warmup} "
                  "warm-ups of each, one process; median of each leg's steps (stream events)",
        **steps,
        "optimizer_launch": optimizer_launch(steps["parameters"], a.kernel_reps, 3, a.kernel_burst),
        "device": torch.cuda.get_device_name(0),
    }
    if a.bench_lines:
        res["bench_py"] = bench_lines(a.bench_lines)
    res["wall_s"] = time.perf_counter() - t0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "step_ms"}))


if __name__ == "__main__":
    main()
