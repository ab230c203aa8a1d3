"""The "reference" against the "model" loss rule (WaveNet.loss_rule) on the config-2 train step, in ONE process.

    python3 scripts/bench_loss_rule.py [--blocks 6] [--steps 5] [--out profiles/loss_rule.json]

The step is bench.py's train leg (config 2: 30 layers, Q = 256, C = K = 64, 16 clips x 16000 samples, the trainer's
fused loss, backward, FlatAdamW).  Three legs alternate in blocks of --steps steps after a warm-up of each, their order
rotating from block to block so that clock and thermal drift fall on all alike: the reference rule, the model rule, and
the reference rule AGAIN -- the two reference legs differ by nothing but their place in the rotation, so the gap between
their medians is the run-to-run spread the model rule's median is read against.  Each step is timed by stream events.

The two loss kernels alone (mvn_softmax_ce_forward_ex / _backward_ex on the step's (16, 256, 12928) head tensor, the
backward into mvn_backward's padded dlogit window) are timed the same way, with HIP events around each launch."""
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
LEGS = (("reference", "reference"), ("model", "model"), ("reference_again", "reference"))


def _median(v):
    return sorted(v)[len(v) // 2]


def train_steps(blocks: int, steps: int, warmup: int) -> dict:
    import torch
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

    times = {leg: [] for leg, _ in LEGS}
    last = {}
    for _, rule in LEGS[:2]:  # warm-up of each rule (allocator, LDS attributes, weight images)
        model.loss_rule = rule
        for _ in range(warmup):
            step()
    torch.cuda.synchronize(dev)
    for blk in range(blocks):
        r = blk % len(LEGS)
        for leg, rule in LEGS[r:] + LEGS[:r]:
            model.loss_rule = rule
            marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
            marks[0].record()
            for i in range(steps):
                loss = step()
                marks[i + 1].record()
            last[leg] = loss.detach()
            torch.cuda.synchronize(dev)
            times[leg] += [marks[i].elapsed_time(marks[i + 1]) for i in range(steps)]
    med = {leg: _median(v) for leg, v in times.items()}
    spread = abs(med["reference"] - med["reference_again"])
    return {
        "step_ms_median": med,
        "step_ms_reference_spread": spread,
        "step_ratio_model_over_reference": med["model"] / min(med["reference"], med["reference_again"]),
        "model_within_spread_or_below": med["model"] <= max(med["reference"], med["reference_again"]),
        "step_ms": {leg: [round(x, 3) for x in v] for leg, v in times.items()},
        "last_loss": {leg: float(v) for leg, v in last.items()},
        "tokens_per_step": BATCH * (T_LEN - rf),
    }


def loss_kernels(reps: int, warmup: int) -> dict:
    """The two loss kernels alone, on the step's shapes: (B, Q, S) logits -> probabilities in place, and the gradient
    into the (B, Q, Sp) window at column (RF - 1) & 31 with the one trailing zero column the trainer asks for."""
    import torch
    from movenet_amd import _native as N
    lib = N.lib()
    dev = torch.device("cuda", 0)
    dims = N.make_dims(*CFG.values())
    rf = lib.mvn_receptive_fields(dims)
    B, Q, S = BATCH, CFG["input_channels"], T_LEN - rf
    Sp, pad = lib.mvn_padded_len(S + 1 + 31), (rf - 1) & 31
    g = torch.Generator(device=dev).manual_seed(3)
    logits = torch.randn(B, Q, S, generator=g, device=dev) * 4.0
    tg = torch.randint(0, Q, (B, S), generator=g, device=dev)
    parts = lib.mvn_ce_parts(B, S)
    lp = torch.zeros(parts, dtype=torch.float32, device=dev)
    cp = torch.zeros(parts, dtype=torch.int32, device=dev)
    up = torch.ones(1, device=dev)
    y = torch.empty_like(logits)
    d = torch.zeros(B, Q, Sp, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rules = {"reference": N.LOSS_REFERENCE, "model": N.LOSS_MODEL}
    out = {"shape": [B, Q, S], "dlogit_ld": Sp, "dlogit_col0": pad, "bytes_each_way": 4 * B * Q * S}
    fwd = {r: [] for r in rules}
    bwd = {r: [] for r in rules}
    for i in range(warmup + reps):
        for name in (("reference", "model") if i % 2 == 0 else ("model", "reference")):
            y.copy_(logits)
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            N.check(lib.mvn_softmax_ce_forward_ex(y.data_ptr(), tg.data_ptr(), B, Q, S, lp.data_ptr(), cp.data_ptr(),
                                                  rules[name], stream), "mvn_softmax_ce_forward_ex")
            e[1].record()
            N.check(lib.mvn_softmax_ce_backward_ex(y.data_ptr(), tg.data_ptr(), B, Q, S, 1.0 / (B * S), up.data_ptr(),
                                                   d.data_ptr(), Q * Sp, Sp, pad, S + 1, rules[name], stream),
                    "mvn_softmax_ce_backward_ex")
            e[2].record()
            torch.cuda.synchronize(dev)
            if i >= warmup:
                fwd[name].append(e[0].elapsed_time(e[1]))
                bwd[name].append(e[1].elapsed_time(e[2]))
    for name in rules:
        f, b = _median(fwd[name]), _median(bwd[name])
        out[name] = {"forward_us": 1e3 * f, "backward_us": 1e3 * b,
                     "forward_GB_per_s": 2 * out["bytes_each_way"] / (f * 1e6),
                     "backward_GB_per_s": 2 * out["bytes_each_way"] / (b * 1e6)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_rule.json"))
    a = ap.parse_args()
    import torch
    t0 = time.perf_counter()
    res = {
        "workload": "config 2 train step (bench.py train leg): 30 layers, Q=256, C=K=64, 16 x 16000, fused loss, "
                    "backward, FlatAdamW",
        "timing": f"{a.blocks} blocks of {a.steps} steps per leg (reference, model, reference again; rotating order) "
                  f"after {a.warmup} warm-ups per rule, one process; median of each leg's steps (stream events)",
        **train_steps(a.blocks, a.steps, a.warmup),
        "loss_kernels": loss_kernels(a.kernel_reps, 3),
        "device": torch.cuda.get_device_name(0),
    }
    res["wall_s"] = time.perf_counter() - t0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "step_ms"}))


if __name__ == "__main__":
    main()
