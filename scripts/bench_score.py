"""What scoring costs (mvn_score_columns, WaveNet.score) on config 2's head tensor, in ONE process.

    python3 scripts/bench_score.py [--reps 30] [--model-reps 7] [--out profiles/score.json]

Kernel legs, on the same (16, 256, 16000 - RF) logits, interleaved (the order rotates from repetition to repetition so
that clock and thermal drift fall on all alike), HIP events around each call, medians:

    score            mvn_score_columns, logp and the per-sequence sums (what WaveNet.score asks for by default)
    score_all        the same call with entropy and rank as well
    loss_forward     the parent's mvn_softmax_ce_forward_ex (MVN_LOSS_MODEL) on a copy of the tensor (the copy is made
                     outside the timed span: the call overwrites its input)
    loss_forward_again   the same leg a second time: the gap between the two medians is that kernel's run-to-run spread
                     in this interleaving, which the score legs are read against
    torch            torch.log_softmax + gather + sum on the GPU

Expectation under test: the score kernel reads the tensor once and writes about 1 % of it, the loss forward reads and
rewrites it, so `score` should be no slower than `loss_forward` beyond that spread.  The JSON says whether it held.

End to end: WaveNet.score against WaveNet.forward (probabilities, no_grad) on 16 x 16000 samples of config 2."""
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


def kernels(reps: int, warmup: int) -> dict:
    import torch
    from movenet_amd import _native as N
    lib = N.lib()
    dev = torch.device("cuda", 0)
    rf = lib.mvn_receptive_fields(N.make_dims(*CFG.values()))
    B, Q, S = BATCH, CFG["input_channels"], T_LEN - rf
    g = torch.Generator(device=dev).manual_seed(3)
    logits = torch.randn(B, Q, S, generator=g, device=dev) * 4.0
    tg = torch.randint(0, Q, (B, S), generator=g, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    logp, ent = torch.empty(B, S, device=dev), torch.empty(B, S, device=dev)
    rank = torch.empty(B, S, dtype=torch.int32, device=dev)
    nll, ok = torch.empty(B, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    n = lib.mvn_score_scratch_floats(B, S)
    scratch = torch.empty(n, device=dev)
    parts = lib.mvn_ce_parts(B, S)
    lp = torch.zeros(parts, device=dev)
    cp = torch.zeros(parts, dtype=torch.int32, device=dev)
    y = torch.empty_like(logits)

    def score(all_outputs):
        N.check(lib.mvn_score_columns(logits.data_ptr(), tg.data_ptr(), B, Q, S, 1.0, logp.data_ptr(),
                                      ent.data_ptr() if all_outputs else None,
                                      rank.data_ptr() if all_outputs else None, nll.data_ptr(), ok.data_ptr(),
                                      scratch.data_ptr(), n, stream), "mvn_score_columns")

    def loss_forward():
        N.check(lib.mvn_softmax_ce_forward_ex(y.data_ptr(), tg.data_ptr(), B, Q, S, lp.data_ptr(), cp.data_ptr(),
                                              N.LOSS_MODEL, stream), "mvn_softmax_ce_forward_ex")

    def torch_leg():
        return torch.log_softmax(logits, 1).gather(1, tg[:, None])[:, 0].sum(1)

    legs = (("score", lambda: score(False), False), ("loss_forward", loss_forward, True),
            ("score_all", lambda: score(True), False), ("loss_forward_again", loss_forward, True),
            ("torch", torch_leg, False))
    times = {name: [] for name, _, _ in legs}
    for i in range(warmup + reps):
        r = i % len(legs)
        for name, call, needs_copy in legs[r:] + legs[:r]:
            if needs_copy:
                y.copy_(logits)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize(dev)
            if i >= warmup:
                times[name].append(e0.elapsed_time(e1))
    med = {name: 1e3 * _median(v) for name, v in times.items()}
    spread = abs(med["loss_forward"] - med["loss_forward_again"])
    tensor_bytes = 4 * B * Q * S
    return {
        "shape": [B, Q, S], "tensor_bytes": tensor_bytes,
        "median_us": med,
        "min_us": {name: 1e3 * min(v) for name, v in times.items()},
        "loss_forward_spread_us": spread,
        "score_GB_per_s": tensor_bytes / (med["score"] * 1e3),
        "loss_forward_GB_per_s": 2 * tensor_bytes / (min(med["loss_forward"], med["loss_forward_again"]) * 1e3),
        "expectation_score_no_slower_than_loss_forward_beyond_its_spread":
            med["score"] <= max(med["loss_forward"], med["loss_forward_again"]) + spread,
        "reps": reps,
    }


def end_to_end(reps: int, warmup: int) -> dict:
    import torch
    from movenet_amd.utils.weights import make_state_dict, one_hot, synthetic_indices
    from movenet_amd.wavenet import WaveNet
    dev = torch.device("cuda", 0)
    model = WaveNet(**CFG)
    model.load_state_dict(make_state_dict(**CFG, seed=0), strict=True)
    model.to(dev).eval()
    Q = CFG["input_channels"]
    audio = one_hot(synthetic_indices(BATCH, T_LEN, Q, 1234).to(dev), Q)

    def forward():
        with torch.no_grad():
            return model(audio)

    legs = (("score", lambda: model.score(audio)), ("forward", forward), ("forward_again", forward))
    times = {name: [] for name, _ in legs}
    for i in range(warmup + reps):
        r = i % len(legs)
        for name, call in legs[r:] + legs[:r]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = call()
            e1.record()
            torch.cuda.synchronize(dev)
            del out
            if i >= warmup:
                times[name].append(e0.elapsed_time(e1))
    med = {name: _median(v) for name, v in times.items()}
    return {"median_ms": med, "forward_spread_ms": abs(med["forward"] - med["forward_again"]),
            "score_over_forward": med["score"] / min(med["forward"], med["forward_again"]), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--model-reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score.json"))
    a = ap.parse_args()
    import torch
    t0 = time.perf_counter()
    res = {
        "workload": "config 2 head tensor (16, 256, 16000 - RF); config 2 model (30 layers, C=K=64), 16 x 16000",
        "timing": "one process, legs interleaved with rotating order, HIP events around each call, medians",
        "kernels": kernels(a.reps, 3),
        "end_to_end": end_to_end(a.model_reps, 2),
        "device": torch.cuda.get_device_name(0),
    }
    res["wall_s"] = time.perf_counter() - t0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
