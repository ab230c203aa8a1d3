"""Cost of classifier-free guidance (mvn_generate_guided) on the FOLD generator at config 2.

    python scripts/bench_guided_generation.py [--steps 4000] [--repeats 5] [--out profiles/guided_generation.json]

The guided step for 8 and for 16 pairs (16 and 32 rows on 8 and 16 pipelines, two turns each) against the unguided
per-sequence step (mvn_generate_seq) for 16 sequences, in one process, interleaved, medians of ``repeats`` runs; us per
step, HIP events.  All three sample under the model rule (T = 1, k = 32, p = 0.9) with a label vector as context.
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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "guided_generation.json"))
    a = ap.parse_args()
    sd = {k: v.to(DEV) for k, v in make_state_dict(**CFG, seed=0).items()}
    T, K, P, scale = 1.0, 32, 0.9, 3.0
    rf = N.lib().mvn_receptive_fields(N.make_dims(**CFG))
    n_total = rf + a.steps * (a.repeats + 1) + 2
    labels = torch.randn(16, CFG["residual_channels"], generator=torch.Generator().manual_seed(0)).to(DEV)

    def gen(batch, **kw):
        g = RingGenerator(**CFG, state_dict=sd, batch=batch, n_total=n_total, device=DEV, variant=N.GEN_FOLD,
                          sampling="model", temperature=[T] * batch, top_k=K, top_p=P, seed=1,
                          global_context=labels[:batch], **kw)
        g.prime(synthetic_indices(1, g.rf, 256, 1234).repeat(batch, 1).to(DEV))
        return g

    runs = {"unguided_16_sequences": gen(16), "guided_8_pairs": gen(8, guidance=scale),
            "guided_16_pairs": gen(16, guidance=scale)}
    for g in runs.values():
        timed(g, a.steps)  # warm-up
    us = {k: [] for k in runs}
    for _ in range(a.repeats):  # interleaved
        for k, g in runs.items():
            us[k].append(timed(g, a.steps))
    for g in runs.values():
        g.check_errors()
    out = {"device": torch.cuda.get_device_name(0), "config": CFG, "variant": "FOLD", "steps": a.steps,
           "repeats": a.repeats, "settings": {"temperature": T, "top_k": K, "top_p": P, "sampling": "model",
                                              "guidance": scale},
           "us_per_step": {k: {"runs": [round(v, 3) for v in vs], "median": round(statistics.median(vs), 3),
                               "min": round(min(vs), 3), "max": round(max(vs), 3)} for k, vs in us.items()}}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
