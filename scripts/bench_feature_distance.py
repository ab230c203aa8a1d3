"""What the spectral distance costs on 1 x MI355X.
  * kernel: stream time of one ``mvn_feature_distance`` call (its two launches, into buffers made beforehand) at
    (16, 80, 63) -- config 2's clip of 16000 samples at hop 256 -- and at (16, 80, 8192), whole rows, by HIP events around
    --calls back-to-back calls (default 50), against the same expression written in torch on the GPU (float64, as the
    definition has it, and float32), the legs taking turns; the two results are compared before anything is timed;
  * sample logger: one logged batch of config 2 under --use_mel (16 clips of 16000 samples, one generated row per clip,
    80 bins, n_fft 1024, hop 256) -- wall time of the ``WaveNet.score`` call ``Dance2Music.score_samples`` makes, and
    of the ``WaveNet.spectral_distance`` call it now makes besides, the two taking turns.
Medians of --rounds rounds (default 7) after a warm-up round.  Writes profiles/feature_distance.json.
Usage: python scripts/bench_feature_distance.py [--rounds R] [--calls N] [--out PATH]"""
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from movenet_amd import _native as N  # noqa: E402
from movenet_amd import ops  # noqa: E402
from movenet_amd.generation import _stream_ptr  # noqa: E402
from movenet_amd.utils.weights import make_state_dict, one_hot, synthetic_indices  # noqa: E402
from movenet_amd.wavenet import WaveNet  # noqa: E402

DEV = torch.device("cuda:0")
C2 = dict(layer_size=10, stack_size=3, input_channels=256, residual_channels=64, skip_channels=64)
SHAPES = ((16, 80, 63), (16, 80, 8192))
DB = 10.0 / math.log(10.0)


def arg(name, default, cast=str):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def stats(xs):
    s = sorted(xs)
    return dict(median=s[len(s) // 2], min=s[0], max=s[-1])


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


def torch_distance(a, b, dtype):
    d = a.to(dtype) - b.to(dtype)
    rms = d.square().mean(1).sqrt()
    return DB * rms.mean(1), d.abs().mean((1, 2))


def kernel(rounds, calls):
    lib = N.lib()
    out = {}

    def events_us(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(calls):
            fn()
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3 / calls
    for B, M, F in SHAPES:
        g = torch.Generator().manual_seed(F)
        a, b = (torch.randn(B, M, F, generator=g).mul_(3.0).to(DEV) for _ in range(2))
        span = torch.tensor([0] * B + [F] * B, dtype=torch.int32, device=DEV)
        lsd, l1 = (torch.empty(B, dtype=torch.float64, device=DEV) for _ in range(2))
        n = int(lib.mvn_feature_distance_scratch_floats(B, F))
        scratch = torch.empty(n // 2, dtype=torch.float64, device=DEV)
        stream = _stream_ptr(DEV)

        def hip():
            N.check(lib.mvn_feature_distance(a.data_ptr(), b.data_ptr(), B, M, F, span.data_ptr(), span[B:].data_ptr(),
                                             lsd.data_ptr(), l1.data_ptr(), None, scratch.data_ptr(), n, stream),
                    "mvn_feature_distance")
        hip()
        want = torch_distance(a, b, torch.float64)
        err = max(float(((lsd - want[0]).abs() / want[0]).max()), float(((l1 - want[1]).abs() / want[1]).max()))
        if not err < 1e-11:
            raise RuntimeError(f"mvn_feature_distance differs from the torch expression by {err:.3e} at {(B, M, F)}")
        seen = interleaved({"mvn_feature_distance": hip, "torch_float64": lambda: torch_distance(a, b, torch.float64),
                            "torch_float32": lambda: torch_distance(a, b, torch.float32)}, rounds, events_us)
        res = {k: stats(v) for k, v in seen.items()}
        res["bytes_read"] = 2 * 4 * B * M * F
        res["read_gb_per_s"] = res["bytes_read"] / (res["mvn_feature_distance"]["median"] * 1e-6) / 1e9
        res["max_rel_difference_from_torch_float64"] = err
        out[f"{B}x{M}x{F}"] = res
    return dict(what=f"stream time of one call, HIP events around {calls} back-to-back calls, us per call", **out)


def sample_logger(rounds):
    torch.manual_seed(3)
    model = WaveNet(**C2, local_channels=80, local_hop=256)
    model.load_state_dict(make_state_dict(**C2, seed=3, gain=2.0, head_gain=6.0), strict=False)
    model.local_conditioning = {"local_channels": 80, "local_hop": 256, "mel_fft": 1024, "mel_fmin": 0.0,
                                "mel_fmax": 8000.0, "audio_rate": 16000}
    model = model.to(DEV).eval()
    B, T, Q = 16, 16000, 256
    src = synthetic_indices(B, T, Q, 1).to(torch.int32).to(DEV)
    gen = synthetic_indices(B, T, Q, 2).to(torch.int32).to(DEV)
    fbank = ops.mel_filterbank(80, 1024, 16000, 0.0, 8000.0)
    feats = ops.logmel(src, Q, 1024, 256, fbank)
    both = torch.cat([one_hot(gen.long().cpu(), Q), one_hot(src.long().cpu(), Q)]).to(DEV)
    both_feats = torch.cat([feats, feats])

    def wall_ms(fn):
        torch.cuda.synchronize(DEV)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(DEV)
        return (time.perf_counter() - t0) * 1e3
    seen = interleaved({"score": lambda: model.score(both, local_features=both_feats, lengths=[T] * (2 * B)),
                        "spectral_distance": lambda: model.spectral_distance(gen, src, lengths=[T] * B)}, rounds, wall_ms)
    res = {k: stats(v) for k, v in seen.items()}
    return dict(what="config 2 under --use_mel, one logged batch of 16 clips x 16000 samples (80 bins, n_fft 1024, hop "
                     "256): the WaveNet.score call of score_samples and the WaveNet.spectral_distance call beside it "
                     "(two logmel launches, the frame span, mvn_feature_distance), wall ms with a synchronise",
                **res, added_share_of_score=res["spectral_distance"]["median"] / res["score"]["median"])


def main() -> None:
    rounds, calls = arg("--rounds", 7, int), arg("--calls", 50, int)
    out_path = arg("--out", os.path.join(ROOT, "profiles", "feature_distance.json"))
    res = dict(device=torch.cuda.get_device_name(DEV), rounds=rounds, calls=calls)
    with torch.cuda.device(DEV):
        res["kernel"] = kernel(rounds, calls)
        res["sample_logger"] = sample_logger(rounds)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
