"""Cost of per-sequence sampling settings (mvn_generate_seq) on the FOLD generator at config 2.

    python scripts/bench_per_sequence_sampling.py [--steps 4000] [--repeats 5] [--out profiles/per_sequence_sampling.json]

1. 16 sampled sequences (model rule, T = 1, k = 32, p = 0.9): the scalar call (mvn_generate_trunc) against the
   per-sequence call with the same settings in every row, interleaved in one process; us per step, HIP events.
2. A 16-point temperature sweep on one prompt: one launch of 16 sequences against 16 launches of one sequence.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from movenet_amd import _native as N  # noqa: E402
from movenet_amd.generation import RingGenerator  # noqa: E402
from movenet_amd.utils.weights import make_state_dict, synthetic_indices  # noqa: E402

CFG = dict(layer_size=10, stack_size=3, input_channels=256, residual_channels=64, skip_channels=64)  # config 2
DEV = "cuda:0"


def timed(g, steps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    g.advance(steps)
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sd = {k: v.to(DEV) for k, v in make_state_dict(**CFG, seed=0).items()}
    B, T, K, P = 16, 1.0, 32, 0.9
    n_total = None

    def gen(batch, **kw):
        nonlocal n_total
        g = RingGenerator(**CFG, state_dict=sd, batch=batch, n_total=n_total, device=DEV, variant=N.GEN_FOLD,
                          sampling="model", **kw)
        g.prime(synthetic_indices(1, g.rf, 256, 1234).repeat(batch, 1).to(DEV))
        return g

    rf = N.lib().mvn_receptive_fields(N.make_dims(**CFG))
    n_total = rf + a.steps * (a.repeats + 1) + 2
    scalar = gen(B, temperature=T, top_k=K, top_p=P, seed=1)
    per_seq = gen(B, temperature=[T] * B, top_k=K, top_p=P, seed=1)
    for g in (scalar, per_seq):
        timed(g, a.steps)  # warm-up
    us = {"scalar": [], "per_sequence": []}
    for _ in range(a.repeats):  # interleaved
        us["scalar"].append(timed(scalar, a.steps))
        us["per_sequence"].append(timed(per_seq, a.steps))
    for g in (scalar, per_seq):
        g.check_errors()
    same = bool(torch.equal(scalar.samples, per_seq.samples))

    temps = [0.1 * (i + 1) for i in range(16)]
    n_total = rf + a.steps * 2 + 2
    one = gen(16, temperature=temps, top_k=K, top_p=P, seed=1)
    singles = [gen(1, temperature=t, top_k=K, top_p=P, seed=1) for t in temps]
    timed(one, a.steps)
    for g in singles:
        timed(g, a.steps // 4)
    sweep_one = timed(one, a.steps) * a.steps
    sweep_16 = sum(timed(g, a.steps) * a.steps for g in singles)
    for g in [one] + singles:
        g.check_errors()
    out = {"device": torch.cuda.get_device_name(0), "config": CFG, "variant": "FOLD", "steps": a.steps,
           "repeats": a.repeats, "settings": {"batch": B, "temperature": T, "top_k": K, "top_p": P, "sampling": "model"},
           "us_per_step": {k: {"runs": [round(v, 3) for v in vs], "median": round(statistics.median(vs), 3),
                               "min": round(min(vs), 3), "max": round(max(vs), 3)} for k, vs in us.items()},
           "per_sequence_samples_equal_scalar": same,
           "sweep_16_temperatures": {"one_launch_ms": round(sweep_one / 1e3, 3),
                                     "sixteen_launches_ms": round(sweep_16 / 1e3, 3),
                                     "ratio": round(sweep_16 / sweep_one, 2)}}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
