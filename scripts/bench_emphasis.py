"""What pre-emphasis and de-emphasis cost against the paths they stand beside, on 1 x MI355X.  The yardstick of every
figure is the parent path in the same process and the same interleaved rounds, never the new code alone.
  * PCM launch: ``mvn_pcm16_deemph_chunk`` against ``mvn_pcm16_chunk`` at 16 rows, n = 1000 / 4000 / 16000 columns, stream
    time of one launch by HIP events, the two taking turns;
  * streamed synthesis: config 2 (30 layers, C = K = 64, Q = 256; FOLD under AUTO), 16 sequences of 16000 new samples,
    ``WaveNet.generate_stream`` at chunk 4000 with ``preemphasis`` 0 and 0.97, wall seconds, the two taking turns after a
    warm-up round;
  * front end: ``ops.audio_frontend`` of 16 stereo clips of 44.1 kHz x 5 s to 160000 frames, Q = 256, with
    ``preemphasis`` 0 and 0.97, stream time of the launch pair by HIP events, the two taking turns.
Medians of --rounds rounds (default 5; the event-timed parts take 4 x as many).  Writes profiles/emphasis.json.
Usage: python scripts/bench_emphasis.py [--rounds R] [--out PATH]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from movenet_amd import ops  # noqa: E402
from movenet_amd.utils.weights import make_state_dict, one_hot, synthetic_indices  # noqa: E402
from movenet_amd.wavenet import MAX_AUDIO_FRAMES, WaveNet  # noqa: E402

DEV = torch.device("cuda:0")
A = 0.97
C2 = dict(layer_size=10, stack_size=3, input_channels=256, residual_channels=64, skip_channels=64)
COLUMNS = (1000, 4000, 16000)


def arg(name, default, cast=str):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def stats(xs):
    s = sorted(xs)
    return dict(median=s[len(s) // 2], min=s[0], max=s[-1])


def event_us(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3


def interleaved(legs, rounds, timer):
    """{name: [timings]} of ``rounds`` rounds after one warm-up round, the order of the legs rotating"""
    names = list(legs)
    seen = {k: [] for k in names}
    for r in range(-1, rounds):
        for name in names[r % len(names):] + names[:r % len(names)]:
            t = timer(legs[name])
            if r >= 0:
                seen[name].append(t)
    return seen


def pcm_launch(rounds):
    Q, B = 256, 16
    samples = synthetic_indices(B, 16000, Q, 7).to(torch.int32).to(DEV)
    state = torch.zeros(B, dtype=torch.float64, device=DEV)
    out = {}
    for n in COLUMNS:
        buf = torch.empty(B, n, dtype=torch.int16, device=DEV)
        seen = interleaved({"pcm16_chunk": lambda: ops.pcm16_chunk(samples, 0, n, Q, out=buf),
                            "pcm16_deemph_chunk": lambda: ops.pcm16_chunk(samples, 0, n, Q, out=buf, deemphasis=A,
                                                                          state=state)}, 4 * rounds, event_us)
        res = {k: stats(v) for k, v in seen.items()}
        res["difference_us"] = res["pcm16_deemph_chunk"]["median"] - res["pcm16_chunk"]["median"]
        out[str(n)] = res
    return dict(what="stream time of one launch, 16 rows x n columns, HIP events, us", **out)


def streamed(rounds):
    model = WaveNet(**C2)
    model.load_state_dict(make_state_dict(**C2, seed=3, gain=2.0, head_gain=6.0), strict=False)
    model = model.to(DEV).eval()
    model.generate_seed = 5
    Q, rf, B, n_new, chunk = 256, model.receptive_fields, 16, 16000, 4000
    prompt = one_hot(synthetic_indices(B, rf, Q, 1234), Q).to(DEV)
    tails = {}

    def leg(a):
        def run():
            model.preemphasis = a
            for _, pcm in model.generate_stream(prompt, n_samples=rf + n_new, temperature=0.0, chunk=chunk):
                last = pcm
            tails[a] = last.copy()
            if model.last_generate_fallback is not None:
                raise RuntimeError("a hand-off timed out and the call fell back: the timings are void")
        return run

    def wall(fn):
        torch.cuda.synchronize(DEV)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(DEV)
        return time.perf_counter() - t0

    seen = interleaved({"plain": leg(0.0), "deemphasis": leg(A)}, rounds, wall)
    model.preemphasis = 0.0
    if np.array_equal(tails[0.0], tails[A]):
        raise RuntimeError("the de-emphasised stream delivered the plain PCM")
    res = {k: stats(v) for k, v in seen.items()}
    plain = res["plain"]
    return dict(what="config 2, 16 sequences x 16000 new samples, greedy, generate_stream at chunk 4000, wall seconds",
                chunks=n_new // chunk, **res, difference_s=res["deemphasis"]["median"] - plain["median"],
                plain_spread_s=plain["max"] - plain["min"])


def front_end(rounds):
    Q, B, rate, seconds = 256, 16, 44100, 5
    rng = np.random.default_rng(3)
    frames = [rate * seconds - 17 * i for i in range(B)]
    pcm = torch.from_numpy(np.concatenate([rng.integers(-20000, 20000, size=2 * f, dtype=np.int16) for f in frames]))
    pcm = pcm.to(DEV)
    desc = torch.from_numpy(ops.audio_clip_descriptors(frames, [2] * B)).to(DEV)

    def leg(a):
        return lambda: ops.audio_frontend(pcm, frames, [2] * B, Q, n_out=MAX_AUDIO_FRAMES, descriptors=desc,
                                          **({"preemphasis": a} if a else {}))
    seen = interleaved({"plain": leg(0.0), "preemphasis": leg(A)}, 4 * rounds, event_us)
    res = {k: stats(v) for k, v in seen.items()}
    return dict(what=f"ops.audio_frontend, 16 stereo clips of {seconds} s at {rate} Hz -> {MAX_AUDIO_FRAMES} frames, "
                     "stream time of the launch pair (with the output allocations), HIP events, us",
                **res, difference_us=res["preemphasis"]["median"] - res["plain"]["median"])


def main() -> None:
    rounds = arg("--rounds", 5, int)
    out_path = arg("--out", os.path.join(ROOT, "profiles", "emphasis.json"))
    res = dict(device=torch.cuda.get_device_name(DEV), coefficient=A, rounds=rounds)
    with torch.cuda.device(DEV):
        res["pcm_launch"] = pcm_launch(rounds)
        res["front_end"] = front_end(rounds)
        res["streamed_synthesis"] = streamed(rounds)
    s, p = res["streamed_synthesis"], res["pcm_launch"]["4000"]
    # the serial kernel against a 4000-step chunk's generation time (the plain stream's wall time per chunk)
    res["deemph_share_of_a_4000_step_chunk"] = p["pcm16_deemph_chunk"]["median"] * 1e-6 / (s["plain"]["median"] / s["chunks"])
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
