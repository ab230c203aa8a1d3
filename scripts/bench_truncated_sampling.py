"""What top-k / top-p truncation of a sampled step costs, on 1 x MI355X, microseconds per step:
  * config 2 (30 layers, C = K = 64, Q = 256) on FOLD, 16 sequences;
  * config 5 (60 layers, C = K = 128, Q = 256) on PIPE_F16, 1 sequence.
Legs per workload: greedy, sampled by the "model" rule (softmax(logits / T), T = 1.0), and that rule with top_k = 32,
with top_p = 0.9, and with both.

One process, one generator state per workload: every leg restores the same primed state, then one launch of --steps
steps is timed with HIP events; the legs are interleaved round by round (their order rotates with the round) after a
warm-up round.  With --parent-lib PATH (a build of libmovenet_hip.so from the parent commit, which has
mvn_generate_ex but no mvn_generate_trunc) that library is loaded beside this build's and runs the same packed weights
and state in the same rounds, TWICE per round: the distance between its two medians is the run-to-run spread the
comparison is read against.  What must hold: greedy and untruncated-sampled of this build within that spread of the
parent's, their samples bit-equal to the parent's.  The truncated legs have no target: their extra cost over the
untruncated sampled step is recorded.
Writes profiles/truncated_sampling_step.json.
Usage: python scripts/bench_truncated_sampling.py [--parent-lib PATH] [--steps N] [--rounds R] [--out PATH]"""
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from movenet_amd import _native as N  # noqa: E402
from movenet_amd.generation import RingGenerator  # noqa: E402
from movenet_amd.utils.weights import make_state_dict, synthetic_indices  # noqa: E402

DEV = torch.device("cuda:0")
WORKLOADS = {
    "config2_fold_16": dict(cfg=dict(layer_size=10, stack_size=3, input_channels=256, residual_channels=64,
                                     skip_channels=64), variant=N.GEN_FOLD, batch=16,
                            what="config 2 (30 layers, C = K = 64, Q = 256), 16 sequences, FOLD"),
    "config5_pipe_f16_1": dict(cfg=dict(layer_size=10, stack_size=6, input_channels=256, residual_channels=128,
                                        skip_channels=128), variant=N.GEN_PIPE_F16, batch=1,
                               what="config 5 (60 layers, C = K = 128, Q = 256), 1 sequence, PIPE_F16"),
}
T_SAMPLED, SEED, TOP_K, TOP_P = 1.0, 5, 32, 0.9
# leg -> (temperature, top_k, top_p), all under the "model" rule
NEW_LEGS = {"greedy": (0.0, 0, 1.0), "sampled_model": (T_SAMPLED, 0, 1.0), "model_top_k": (T_SAMPLED, TOP_K, 1.0),
            "model_top_p": (T_SAMPLED, 0, TOP_P), "model_top_k_top_p": (T_SAMPLED, TOP_K, TOP_P)}
PARENT_LEGS = ("greedy", "sampled_model")


def arg(name, default, cast=str):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def load_parent(path):
    lib = C.CDLL(path)
    lib.mvn_generate_ex.restype, lib.mvn_generate_ex.argtypes = N.SIGNATURES["mvn_generate_ex"]
    lib.mvn_last_error.restype = C.c_char_p
    return lib


def stats(xs):
    s = sorted(xs)
    return dict(median=s[len(s) // 2], min=s[0], max=s[-1])


def run_workload(lib, parent, cfg, variant, batch, what, steps, rounds):
    sd = {k: v.to(DEV) for k, v in make_state_dict(**cfg, seed=3, gain=2.0, head_gain=6.0).items()}
    g = RingGenerator(**cfg, state_dict=sd, batch=batch, n_total=6144 + steps + 2, device=DEV, variant=variant)
    rf = g.rf
    g.prime(synthetic_indices(batch, rf, 256, 1234).to(DEV))
    g.check_errors()
    state0, samples0, t0 = g.state.clone(), g.samples.clone(), g.t
    stream = torch.cuda.current_stream(DEV).cuda_stream

    def launch(which, temperature, top_k, top_p):
        head = (g.dims, g.variant, g.packed.data_ptr(), g.state.data_ptr(), g.samples.data_ptr(), batch,
                g.samples.stride(0), g.n_total, rf, t0, t0 + steps, temperature, SEED, None, None, 0, None,
                N.SAMPLE_MODEL)
        if which == "parent":
            rc = parent.mvn_generate_ex(*head, stream)
            if rc:
                raise RuntimeError(f"parent mvn_generate_ex: {parent.mvn_last_error().decode()} (status {rc})")
        else:
            N.check(lib.mvn_generate_trunc(*head, top_k, top_p, stream), "mvn_generate_trunc")

    legs = {k: ("new",) + v for k, v in NEW_LEGS.items()}
    if parent is not None:
        for run in ("a", "b"):
            for leg in PARENT_LEGS:
                legs[f"parent_{run}_{leg}"] = ("parent",) + NEW_LEGS[leg]
    names = list(legs)
    us = {k: [] for k in names}
    result = {}
    for r in range(-1, rounds):  # round -1: warm-up (code objects loaded, weights in place), not recorded
        order = names[r % len(names):] + names[:r % len(names)]
        marks = []
        for name in order:
            g.state.copy_(state0)
            g.samples.copy_(samples0)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            launch(*legs[name])
            ev[1].record()
            marks.append((name, ev))
            if r == rounds - 1:
                result[name] = g.samples.clone()
        torch.cuda.synchronize(DEV)
        if int(g.status_word()[0].item()) != 0:
            raise RuntimeError("a hand-off timed out (pipeline stages not co-resident): the timings are void")
        if r >= 0:
            for name, ev in marks:
                us[name].append(ev[0].elapsed_time(ev[1]) * 1e3 / steps)

    res = dict(workload=f"{what}, {steps} steps per launch, {rounds} interleaved rounds, HIP events, \"model\" rule, "
                        f"T = {T_SAMPLED} on the sampled legs, top_k = {TOP_K}, top_p = {TOP_P}",
               new={k: stats(us[k]) for k in NEW_LEGS}, parent=None)
    base = res["new"]["sampled_model"]["median"]
    res["truncation_extra_us"] = {k: res["new"][k]["median"] - base for k in NEW_LEGS if k.startswith("model_top")}
    res["truncation_extra_over_sampled_step"] = {k: v / base for k, v in res["truncation_extra_us"].items()}
    res["distinct_classes_drawn"] = {k: int(torch.unique(result[k][:, rf:rf + steps]).numel()) for k in NEW_LEGS}
    if parent is not None:
        par, spread, checks = {}, {}, {}
        for leg in PARENT_LEGS:
            a, b = stats(us[f"parent_a_{leg}"]), stats(us[f"parent_b_{leg}"])
            par[leg] = dict(run_a=a, run_b=b, median=(a["median"] + b["median"]) / 2)
            spread[leg] = abs(a["median"] - b["median"])
            if not (torch.equal(result[leg], result[f"parent_a_{leg}"]) and
                    torch.equal(result[leg], result[f"parent_b_{leg}"])):
                raise RuntimeError(f"{leg}: this build's samples differ from the parent's")
            diff = res["new"][leg]["median"] - par[leg]["median"]
            checks[f"{leg}_minus_parent"] = diff
            checks[f"{leg}_within_spread"] = abs(diff) <= spread[leg]
        res.update(parent=par, parent_run_to_run_spread=spread, checks=checks, samples_bit_equal_to_parent=True)
    return res


def main() -> None:
    steps, rounds = arg("--steps", 4000, int), arg("--rounds", 15, int)
    parent_path = arg("--parent-lib", None)
    out_path = arg("--out", os.path.join(ROOT, "profiles", "truncated_sampling_step.json"))
    lib, parent = N.lib(), load_parent(parent_path) if parent_path else None
    res = dict(device=torch.cuda.get_device_name(DEV), unit="us per step")
    if parent is None:
        res["note"] = "no --parent-lib given: this build only, nothing to compare against"
    with torch.cuda.device(DEV):
        for name, w in WORKLOADS.items():
            res[name] = run_workload(lib, parent, w["cfg"], w["variant"], w["batch"], w["what"], steps, rounds)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
