"""What the step-closing choice costs on the FOLD generator, on 1 x MI355X: config 2 (30 layers, C = K = 64, Q = 256),
16 sequences, microseconds per step for greedy decoding, sampling by the reference rule (softmax(softmax(logits) / T))
and sampling by the model rule (softmax(logits / T)) at T = 1.0.

One process, one generator state: every leg restores the same primed state, then one launch of --steps steps is timed
with HIP events; the legs are interleaved round by round (their order rotates with the round) after a warm-up round.
With --parent-lib PATH (a build of libmovenet_hip.so from the parent commit, which has mvn_generate only) that library
is loaded beside this build's and runs the same packed weights and state in the same rounds, TWICE per round: the
distance between its two medians is the run-to-run spread the comparison is read against.  What must hold:
greedy and sampled-reference of this build within that spread of the parent's, sampled-model no slower than the
parent's sampled-reference beyond it.  The samples of corresponding legs must be bit-equal.
Writes profiles/sampling_step.json.
Usage: python scripts/bench_sampling.py [--parent-lib PATH] [--steps N] [--rounds R] [--out PATH]"""
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
CFG = dict(layer_size=10, stack_size=3, input_channels=256, residual_channels=64, skip_channels=64)
B, T_SAMPLED, SEED = 16, 1.0, 5


def arg(name, default, cast=str):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def load_parent(path):
    lib = C.CDLL(path)
    lib.mvn_generate.restype, lib.mvn_generate.argtypes = N.SIGNATURES["mvn_generate"]
    lib.mvn_last_error.restype = C.c_char_p
    return lib


def stats(xs):
    s = sorted(xs)
    return dict(median=s[len(s) // 2], min=s[0], max=s[-1])


def main() -> None:
    steps, rounds = arg("--steps", 4000, int), arg("--rounds", 15, int)
    parent_path = arg("--parent-lib", None)
    out_path = arg("--out", os.path.join(ROOT, "profiles", "sampling_step.json"))
    lib, parent = N.lib(), load_parent(parent_path) if parent_path else None
    with torch.cuda.device(DEV):
        sd = {k: v.to(DEV) for k, v in make_state_dict(**CFG, seed=3, gain=2.0, head_gain=6.0).items()}
        g = RingGenerator(**CFG, state_dict=sd, batch=B, n_total=3072 + steps + 2, device=DEV, variant=N.GEN_FOLD)
        rf = g.rf
        g.prime(synthetic_indices(B, rf, 256, 1234).to(DEV))
        g.check_errors()
        state0, samples0, t0 = g.state.clone(), g.samples.clone(), g.t
        stream = torch.cuda.current_stream(DEV).cuda_stream

        def launch(which, temperature, sampling):
            head = (g.dims, g.variant, g.packed.data_ptr(), g.state.data_ptr(), g.samples.data_ptr(), B,
                    g.samples.stride(0), g.n_total, rf, t0, t0 + steps, temperature, SEED, None, None, 0, None)
            if which == "parent":
                rc = parent.mvn_generate(*head, stream)
                if rc:
                    raise RuntimeError(f"parent mvn_generate: {parent.mvn_last_error().decode()} (status {rc})")
            else:
                N.check(lib.mvn_generate_ex(*head, sampling, stream), "mvn_generate_ex")

        legs = {"greedy": ("new", 0.0, N.SAMPLE_REFERENCE), "sampled_reference": ("new", T_SAMPLED, N.SAMPLE_REFERENCE),
                "sampled_model": ("new", T_SAMPLED, N.SAMPLE_MODEL)}
        if parent is not None:
            for run in ("a", "b"):
                legs[f"parent_{run}_greedy"] = ("parent", 0.0, 0)
                legs[f"parent_{run}_sampled_reference"] = ("parent", T_SAMPLED, 0)
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

    res = dict(workload=f"config 2 (30 layers, C = K = 64, Q = 256), {B} sequences, FOLD, {steps} steps per launch, "
                        f"{rounds} interleaved rounds, HIP events, T = {T_SAMPLED} on the sampled legs",
               device=torch.cuda.get_device_name(DEV), unit="us per step",
               new={k: stats(us[k]) for k in ("greedy", "sampled_reference", "sampled_model")}, parent=None)
    if parent is None:
        res["note"] = "no --parent-lib given: this build only, nothing to compare against"
    else:
        par, spread, checks = {}, {}, {}
        for leg in ("greedy", "sampled_reference"):
            a, b = stats(us[f"parent_a_{leg}"]), stats(us[f"parent_b_{leg}"])
            par[leg] = dict(run_a=a, run_b=b, median=(a["median"] + b["median"]) / 2)
            spread[leg] = abs(a["median"] - b["median"])
            if not (torch.equal(result[leg], result[f"parent_a_{leg}"]) and
                    torch.equal(result[leg], result[f"parent_b_{leg}"])):
                raise RuntimeError(f"{leg}: this build's samples differ from the parent's")
            diff = res["new"][leg]["median"] - par[leg]["median"]
            checks[f"{leg}_minus_parent"] = diff
            checks[f"{leg}_within_spread"] = abs(diff) <= spread[leg]
        diff = res["new"]["sampled_model"]["median"] - par["sampled_reference"]["median"]
        checks["sampled_model_minus_parent_sampled_reference"] = diff
        checks["sampled_model_no_slower_beyond_spread"] = diff <= spread["sampled_reference"]
        res.update(parent=par, parent_run_to_run_spread=spread, checks=checks,
                   samples_bit_equal_to_parent=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
