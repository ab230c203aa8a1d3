"""What the F0 conditioning channels cost on 1 x MI355X.
  * kernel: stream time of one ``mvn_pitch_features`` call (one launch, into a tensor made beforehand) at (16, 63)
    frames -- config 2's batch at hop 256 -- and at (16, 8192), by HIP events around --calls back-to-back calls, against
    the same expression written in torch on the GPU (cummax / cummin, two gathers, a lerp, the wheres), the legs taking
    turns; the two results are compared before anything is timed;
  * features: wall time of ``ops.local_features`` on config 2's batch (16 clips of 16000 samples, 80 bins, mel_fft 1024,
    hop 256) without and with an ``"f0"`` entry in the record;
  * step: features, ``forward(return_loss=True)`` and ``backward`` of config 2 under --use_mel on that batch, with
    ``local_channels`` 80 and 82 (no optimizer step: it does not see the two columns' cost apart from 128 more weights).
Medians of --rounds rounds (default 7) after a warm-up round.  Writes profiles/f0_features.json.
Usage: python scripts/bench_f0_features.py [--rounds R] [--calls N] [--out PATH]"""
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
RATE, F_MIN, F_MAX = 16000, 60.0, 500.0
F_REF = math.sqrt(F_MIN * F_MAX)
RECORD = {"local_channels": 80, "local_hop": 256, "mel_fft": 1024, "mel_fmin": 0.0, "mel_fmax": 8000.0,
          "audio_rate": RATE}
RECORD_F0 = {**RECORD, "f0": {"f_min": F_MIN, "f_max": F_MAX, "f_ref": F_REF}}
SHAPES = ((16, 63), (16, 8192))


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


def torch_features(period, rate, f_ref):
    """(B, F) periods -> (B, 2, F): the definition of mvn_pitch_features as torch has it."""
    B, F = period.shape
    v = period > 0
    j = torch.arange(F, device=period.device)[None].expand(B, F)
    prev = torch.where(v, j, torch.full_like(j, -1)).cummax(1).values
    nxt = torch.where(v, j, torch.full_like(j, F)).flip(1).cummin(1).values.flip(1)
    lf = torch.where(v, torch.log2(rate / (period.double() * f_ref)).float(), torch.zeros_like(period))
    lp, ln = lf.gather(1, prev.clamp(min=0)), lf.gather(1, nxt.clamp(max=F - 1))
    a = (j - prev).float() / (nxt - prev).float()
    lerp = a * ln + (1.0 - a) * lp
    held = torch.where(prev < 0, torch.where(nxt >= F, torch.zeros_like(lf), ln), torch.where(nxt >= F, lp, lerp))
    return torch.stack([torch.where(v, lf, held), v.float()], 1)


def wall_ms(fn):
    torch.cuda.synchronize(DEV)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(DEV)
    return (time.perf_counter() - t0) * 1e3


def kernel(rounds, calls):
    lib = N.lib()
    out = {}

    def events_us(fn, n=calls):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(n):
            fn()
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3 / n
    for B, F in SHAPES:
        g = torch.Generator().manual_seed(F)
        period = RATE / F_MAX + (RATE / F_MIN - RATE / F_MAX) * torch.rand(B, F, generator=g)
        period[torch.rand(B, F, generator=g) < 0.4] = 0.0          # unvoiced frames, singly and in runs
        period[:, F // 3:F // 3 + F // 8] = 0.0
        period = period.to(DEV)
        res = torch.empty(B, 2, F, dtype=torch.float32, device=DEV)
        stream = _stream_ptr(DEV)

        def hip():
            N.check(lib.mvn_pitch_features(period.data_ptr(), B, F, float(RATE), F_REF, None, res.data_ptr(), 2 * F, F,
                                           stream), "mvn_pitch_features")
        hip()
        torch.cuda.synchronize(DEV)
        want = torch_features(period, float(RATE), F_REF)
        err = float((res - want).abs().max())
        if not err < 1e-5:
            raise RuntimeError(f"mvn_pitch_features differs from the torch expression by {err:.3e} at {(B, F)}")
        seen = interleaved({"mvn_pitch_features": hip,
                            "torch_scan_gather_lerp": lambda: torch_features(period, float(RATE), F_REF)}, rounds,
                           events_us)
        out[f"{B}x{F}"] = {**{k: stats(v) for k, v in seen.items()}, "max_abs_difference_from_torch": err}
    return dict(what=f"stream time of one call, HIP events around {calls} back-to-back calls, us per call", **out)


def features_and_step(rounds):
    B, T, Q = 16, 16000, 256
    idx = synthetic_indices(B, T, Q, 1).to(torch.int32).to(DEV)
    audio = one_hot(idx.long().cpu(), Q).to(DEV)
    feats = {"mel": lambda: ops.local_features(idx, Q, RECORD), "mel_f0": lambda: ops.local_features(idx, Q, RECORD_F0)}
    res = {"local_features": {k: stats(v) for k, v in interleaved(feats, rounds, wall_ms).items()}}
    models = {}
    for name, rec in (("mel", RECORD), ("mel_f0", RECORD_F0)):
        torch.manual_seed(3)
        M = int(feats[name]().shape[1])
        m = WaveNet(**C2, local_channels=M, local_hop=256)
        m.load_state_dict(make_state_dict(**C2, seed=3, gain=1.0), strict=False)
        models[name] = m.to(DEV).train()

    def step(name):
        def run():
            m = models[name]
            for p in m.parameters():
                p.grad = None
            loss, _, _ = m(audio, return_loss=True, local_features=feats[name]())
            loss.backward()
        return run
    seen = interleaved({k: step(k) for k in models}, rounds, wall_ms)
    res["step"] = {k: stats(v) for k, v in seen.items()}
    res["what"] = ("config 2 under --use_mel, 16 clips x 16000 samples, wall ms with a synchronise: ops.local_features, "
                   "and features + forward(return_loss=True) + backward, without and with the record's f0 entry")
    return res


def main() -> None:
    rounds, calls = arg("--rounds", 7, int), arg("--calls", 20, int)
    out_path = arg("--out", os.path.join(ROOT, "profiles", "f0_features.json"))
    res = dict(device=torch.cuda.get_device_name(DEV), rounds=rounds, calls=calls)
    with torch.cuda.device(DEV):
        res["kernel"] = kernel(rounds, calls)
        res["config2"] = features_and_step(rounds)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
