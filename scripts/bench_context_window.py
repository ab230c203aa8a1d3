"""What the windowed generator context costs and saves against the whole context, on 1 x MI355X:
  (a) config 2 (30 layers, C = K = 64, Q = 256; FOLD under AUTO), 16 sequences x 16000 new samples under log-mel frames
      (80 mels, hop 256), ``WaveNet.generate_stream`` at chunk 4000, sampled by the model rule: ``context="whole"``
      against ``context="windowed"`` -- wall seconds, seconds to the first GENERATED chunk, and
      ``torch.cuda.max_memory_allocated`` of the call; one ``mvn_context_window`` launch between HIP events at
      n = 1000, 4000 and 16000;
  (b) one sequence x 960 000 new samples (one minute at 16 kHz), windowed only: peak memory, and microseconds per step
      against (a)'s.
One process; after a warm-up round the legs of (a) are interleaved round by round, their order alternating; medians of
--rounds rounds (default 5).  The yardstick for time is the whole-context leg in the same process and rounds.
Writes profiles/context_window.json.
Usage: python scripts/bench_context_window.py [--rounds R] [--out PATH] [--long_columns N]"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from movenet_amd import ops  # noqa: E402
from movenet_amd.utils.weights import make_state_dict, one_hot, synthetic_indices  # noqa: E402
from movenet_amd.wavenet import WaveNet  # noqa: E402

DEV = torch.device("cuda:0")
CFG = dict(layer_size=10, stack_size=3, input_channels=256, residual_channels=64, skip_channels=64)
MELS, HOP, CHUNK = 80, 256, 4000


def arg(name, default, cast=str):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def stats(xs):
    s = sorted(xs)
    return dict(median=s[len(s) // 2], min=s[0], max=s[-1])


def make_model():
    torch.manual_seed(29)
    model = WaveNet(**CFG, local_channels=MELS, local_hop=HOP)
    model.load_state_dict(make_state_dict(**CFG, seed=3, gain=2.0, head_gain=6.0), strict=False)
    model = model.to(DEV).eval()
    model.generate_sampling, model.generate_top_k, model.generate_top_p, model.generate_seed = "model", 32, 0.9, 5
    return model


def stream(model, prompt, feats, n_total, context):
    """One call: wall seconds, seconds to the first generated chunk, peak bytes allocated during it, the last chunk."""
    model.generate_local_features = feats
    torch.cuda.synchronize(DEV)
    torch.cuda.reset_peak_memory_stats(DEV)
    before = torch.cuda.memory_allocated(DEV)
    t0 = time.perf_counter()
    first, last = None, None
    for at, pcm in model.generate_stream(prompt, n_samples=n_total, temperature=1.0, chunk=CHUNK, context=context):
        if at > 0 and first is None:
            first = time.perf_counter() - t0
        last = pcm
    torch.cuda.synchronize(DEV)
    wall = time.perf_counter() - t0
    if model.last_generate_fallback is not None:
        raise RuntimeError("a hand-off timed out and the call fell back: the timings are void")
    peak = torch.cuda.max_memory_allocated(DEV)
    return dict(wall=wall, first_chunk=first, peak_bytes=peak, peak_above_start_bytes=peak - before), last.copy()


def main() -> None:
    rounds = arg("--rounds", 5, int)
    long_columns = arg("--long_columns", 960000, int)
    out_path = arg("--out", os.path.join(ROOT, "profiles", "context_window.json"))
    res = dict(device=torch.cuda.get_device_name(DEV))
    with torch.cuda.device(DEV):
        model = make_model()
        Q, rf, C = CFG["input_channels"], model.receptive_fields, CFG["residual_channels"]
        # ---- (a) 16 x 16000, whole against windowed ----
        B, n_new = 16, 16000
        n_total = rf + n_new
        prompt = one_hot(synthetic_indices(B, rf, Q, 1234), Q).to(DEV)
        feats = torch.randn(B, MELS, (n_total - 1) // HOP + 1, generator=torch.Generator().manual_seed(5)).to(DEV)
        legs = ["whole", "windowed"]
        seen, tails = {k: [] for k in legs}, {}
        for r in range(-1, rounds):  # round -1: warm-up (code objects, calibration, pinned buffers), not recorded
            for name in (legs if r % 2 == 0 else legs[::-1]):
                got, tail = stream(model, prompt, feats, n_total, name)
                if r >= 0:
                    seen[name].append(got)
                tails[name] = tail
        if not (tails["whole"] == tails["windowed"]).all():
            raise RuntimeError("the windowed leg's last chunk differs from the whole-context leg's")
        a = dict(workload=f"config 2, {B} sequences x {n_new} new samples, {MELS} mels at hop {HOP}, chunk {CHUNK}, model "
                          f"rule T = 1 k = 32 p = 0.9; {rounds} interleaved rounds after one warm-up round")
        for name in legs:
            xs = seen[name]
            wall = stats([x["wall"] for x in xs])
            a[name] = dict(wall_s=wall, us_per_step=wall["median"] / n_new * 1e6,
                           first_generated_chunk_s=stats([x["first_chunk"] for x in xs]),
                           peak_bytes=stats([x["peak_bytes"] for x in xs]),
                           peak_above_start_bytes=stats([x["peak_above_start_bytes"] for x in xs]))
        a["windowed_minus_whole_wall_s"] = a["windowed"]["wall_s"]["median"] - a["whole"]["wall_s"]["median"]
        a["whole_round_to_round_spread_s"] = a["whole"]["wall_s"]["max"] - a["whole"]["wall_s"]["min"]
        res["a_config2_16x16000"] = a
        # one mvn_context_window launch per window width, HIP events
        proj = ops.project_features(model, feats)
        launches = {}
        for n in (1000, 4000, 16000):
            buf = torch.empty(B * n * C, device=DEV)
            times = []
            for i in range(25):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                ops.context_window(proj, HOP, rf - 1, n, out=buf)
                ev[1].record()
                ev[1].synchronize()
                if i >= 5:
                    times.append(ev[0].elapsed_time(ev[1]) * 1e3)
            launches[str(n)] = dict(rows=B, columns=n, bytes_written=4 * B * n * C, **stats(times))
        res["context_window_launch_us"] = launches
        del proj, buf, feats, prompt
        # ---- (b) one sequence, one minute, windowed only ----
        n_total = rf + long_columns
        prompt = one_hot(synthetic_indices(1, rf, Q, 1234), Q).to(DEV)
        feats = torch.randn(1, MELS, (n_total - 1) // HOP + 1, generator=torch.Generator().manual_seed(6)).to(DEV)
        got, _ = stream(model, prompt, feats, n_total, "windowed")
        res["b_one_sequence_long"] = dict(
            workload=f"config 2, 1 sequence x {long_columns} new samples, windowed, chunk {CHUNK}; one run",
            wall_s=got["wall"], us_per_step=got["wall"] / long_columns * 1e6, first_generated_chunk_s=got["first_chunk"],
            peak_bytes=got["peak_bytes"], peak_above_start_bytes=got["peak_above_start_bytes"],
            whole_context_would_take_bytes=2 * C * n_total * 4,
            us_per_step_of_a_windowed=a["windowed"]["us_per_step"], us_per_step_of_a_whole=a["whole"]["us_per_step"])
    res["not_measured"] = ["long runs at batch 16", "python -m movenet_amd.synthesize end to end on a real recording"]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
