"""What handing audio out in chunks costs against generating the whole clip, on 1 x MI355X, wall seconds per call:
  * config 2 (30 layers, C = K = 64, Q = 256; FOLD under AUTO), 16 sequences of 16000 new samples;
  * config 5 (60 layers, C = K = 128, Q = 256; PIPE_F16), 1 sequence of 22050 new samples.
Legs per workload, all through the model's own entry points with the same prompt, seed and greedy decoding:
``WaveNet.generate`` (which also forms the (B, Q, T) one-hot result), and ``WaveNet.generate_stream`` at chunk 1000,
4000 and 16000, the consumer doing nothing with a chunk.  Per streamed leg also the time from the call to the first
GENERATED chunk (the prompt's chunk comes before it).  One process; after a warm-up round the legs are interleaved
round by round, their order rotating; medians of --rounds rounds (default 5).  The stream time of one
``mvn_pcm16_chunk`` launch per chunk size is timed apart, with HIP events.
The baseline of "streaming costs nothing" is ``generate`` in the same process and rounds.
Writes profiles/stream_synthesis.json.
Usage: python scripts/bench_stream_synthesis.py [--rounds R] [--out PATH]"""
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
WORKLOADS = {
    "config2_fold_16": dict(cfg=dict(layer_size=10, stack_size=3, input_channels=256, residual_channels=64,
                                     skip_channels=64), precision="fp32", batch=16, n_new=16000,
                            what="config 2 (30 layers, C = K = 64, Q = 256), 16 sequences x 16000 new samples, AUTO (FOLD)"),
    "config5_pipe_f16_1": dict(cfg=dict(layer_size=10, stack_size=6, input_channels=256, residual_channels=128,
                                        skip_channels=128), precision="fp16", batch=1, n_new=22050,
                               what="config 5 (60 layers, C = K = 128, Q = 256), 1 sequence x 22050 new samples, PIPE_F16"),
}
CHUNKS = (1000, 4000, 16000)


def arg(name, default, cast=str):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def stats(xs):
    s = sorted(xs)
    return dict(median=s[len(s) // 2], min=s[0], max=s[-1])


def run_workload(cfg, precision, batch, n_new, what, rounds):
    model = WaveNet(**cfg)
    model.load_state_dict(make_state_dict(**cfg, seed=3, gain=2.0, head_gain=6.0), strict=False)
    model = model.to(DEV).eval()
    model.generate_precision = precision
    model.generate_seed = 5
    Q, rf = cfg["input_channels"], model.receptive_fields
    prompt = one_hot(synthetic_indices(batch, rf, Q, 1234), Q).to(DEV)
    n_total = rf + n_new

    def whole():
        torch.cuda.synchronize(DEV)
        t0 = time.perf_counter()
        out = model.generate(prompt, n_samples=n_total, temperature=0.0)
        torch.cuda.synchronize(DEV)
        return dict(wall=time.perf_counter() - t0), out.argmax(1)

    def streamed(chunk):
        torch.cuda.synchronize(DEV)
        t0 = time.perf_counter()
        first, n_chunks, last = None, 0, None
        for at, pcm in model.generate_stream(prompt, n_samples=n_total, temperature=0.0, chunk=chunk):
            if at > 0:
                n_chunks += 1
                if first is None:
                    first = time.perf_counter() - t0
            last = pcm
        torch.cuda.synchronize(DEV)
        return dict(wall=time.perf_counter() - t0, first_chunk=first, chunks=n_chunks), last.copy()

    legs = {"generate": whole, **{f"stream_{c}": (lambda c=c: streamed(c)) for c in CHUNKS}}
    names = list(legs)
    seen = {k: [] for k in names}
    tails = {}
    for r in range(-1, rounds):  # round -1: warm-up (code objects, calibration, pinned buffers), not recorded
        for name in names[r % len(names):] + names[:r % len(names)]:
            res, tail = legs[name]()
            if model.last_generate_fallback is not None:
                raise RuntimeError("a hand-off timed out and the call fell back: the timings are void")
            if r >= 0:
                seen[name].append(res)
            tails[name] = tail
    # the streamed legs delivered generate()'s samples
    want = ops.pcm16_chunk(tails["generate"].to(torch.int32), 0, n_total, Q).cpu().numpy()
    for c in CHUNKS:
        tail = tails[f"stream_{c}"]
        if not (tail == want[:, n_total - tail.shape[1]:]).all():
            raise RuntimeError(f"stream_{c}: the last chunk differs from generate()'s samples")
    out = dict(workload=f"{what}; greedy, {rounds} interleaved rounds after one warm-up round, wall seconds",
               generate=dict(wall_s=stats([x["wall"] for x in seen["generate"]])))
    base = out["generate"]["wall_s"]["median"]
    for c in CHUNKS:
        xs = seen[f"stream_{c}"]
        wall = stats([x["wall"] for x in xs])
        out[f"stream_{c}"] = dict(wall_s=wall, first_generated_chunk_s=stats([x["first_chunk"] for x in xs]),
                                  chunks=xs[0]["chunks"], wall_minus_generate_s=wall["median"] - base,
                                  wall_minus_generate_per_chunk_us=(wall["median"] - base) / xs[0]["chunks"] * 1e6)
    # one mvn_pcm16_chunk launch per chunk size, HIP events
    samples = synthetic_indices(batch, n_total, Q, 7).to(torch.int32).to(DEV)
    pcm_us = {}
    for c in CHUNKS:
        n = min(c, n_new)
        buf = torch.empty(batch, n, dtype=torch.int16, device=DEV)
        times = []
        for i in range(25):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            ops.pcm16_chunk(samples, rf, n, Q, out=buf)
            ev[1].record()
            ev[1].synchronize()
            if i >= 5:
                times.append(ev[0].elapsed_time(ev[1]) * 1e3)
        pcm_us[str(c)] = dict(columns=n, **stats(times))
    out["pcm16_chunk_stream_us"] = pcm_us
    return out


def main() -> None:
    rounds = arg("--rounds", 5, int)
    out_path = arg("--out", os.path.join(ROOT, "profiles", "stream_synthesis.json"))
    res = dict(device=torch.cuda.get_device_name(DEV), unit="wall seconds per call unless a key says otherwise")
    with torch.cuda.device(DEV):
        for name, w in WORKLOADS.items():
            res[name] = run_workload(w["cfg"], w["precision"], w["batch"], w["n_new"], w["what"], rounds)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
