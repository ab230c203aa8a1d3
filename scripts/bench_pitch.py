"""What the pitch tracker costs on 1 x MI355X.
  * kernel: stream time of one ``mvn_pitch_frames`` call on a float32 waveform (one launch, into buffers made beforehand,
    no cmnd) at 16 x 16000 samples -- config 2's clip -- and at 16 x 2^20, with win 1024, hop 256 and the lags of
    60 .. 500 Hz at 16 kHz (32 .. 267), by HIP events around --calls back-to-back calls, against the same expression
    written in torch on the GPU at the first shape (unfold + broadcast: a (B, F, win, tau_max) intermediate, the pick
    left out), the legs taking turns; c of the two is compared before anything is timed;
  * sample logger: one logged batch of config 2 under --use_mel (16 clips of 16000 samples, one generated row per clip) --
    wall time of the ``WaveNet.score`` call ``Dance2Music.score_samples`` makes, of its ``WaveNet.spectral_distance`` call
    and of the ``WaveNet.pitch_distance`` call ``--score_pitch 1`` adds, the three taking turns.
Medians of --rounds rounds (default 7) after a warm-up round.  Writes profiles/pitch.json.
Usage: python scripts/bench_pitch.py [--rounds R] [--calls N] [--out PATH]"""
import json
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
WIN, HOP, RATE = 1024, 256, 16000
SHAPES = ((16, 16000), (16, 1 << 20))


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


def torch_cmnd(x, win, hop, tau_max):
    """c(1 .. tau_max) of every frame, (B, F, tau_max), as torch has it: the padded rows unfolded into frames, the frames
    into lagged windows, one broadcast difference."""
    L = win + tau_max
    F = x.shape[1] // hop + 1
    pad_front = L // 2
    pad_back = (F - 1) * hop - pad_front + L - x.shape[1]
    frames = torch.nn.functional.pad(x, (pad_front, max(pad_back, 0))).unfold(1, L, hop)[:, :F]  # (B, F, L)
    lagged = frames.unfold(2, win, 1)                                                          # (B, F, tau_max + 1, win)
    d = (lagged[:, :, :1] - lagged[:, :, 1:]).square().sum(3)                                    # (B, F, tau_max)
    run = d.cumsum(2)
    tau = torch.arange(1, tau_max + 1, device=x.device, dtype=x.dtype)
    return torch.where(run > 0, d * tau / run, torch.ones_like(d))


def kernel(rounds, calls):
    lib = N.lib()
    tau_min, tau_max = ops.pitch_lags(RATE, 60.0, 500.0)
    out = {}

    def events_us(fn, n=calls):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(n):
            fn()
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3 / n
    for B, T in SHAPES:
        g = torch.Generator().manual_seed(T)
        t = torch.arange(T, dtype=torch.float32)
        x = (0.5 * torch.sin(2 * torch.pi * t / 97.3)[None] + 0.1 * torch.randn(B, T, generator=g)).to(DEV)
        F = T // HOP + 1
        period, aper = (torch.empty(B, F, dtype=torch.float32, device=DEV) for _ in range(2))
        n = int(lib.mvn_pitch_scratch_floats(B, T, WIN, tau_max))
        scratch = torch.empty(n, dtype=torch.float32, device=DEV)
        stream = _stream_ptr(DEV)

        def hip():
            N.check(lib.mvn_pitch_frames(None, x.data_ptr(), B, T, 0, WIN, HOP, tau_min, tau_max, 0.15, period.data_ptr(),
                                         aper.data_ptr(), None, scratch.data_ptr(), n, stream), "mvn_pitch_frames")
        legs = {"mvn_pitch_frames": hip}
        res = {}
        if T == SHAPES[0][1]:
            c = ops.pitch(x, win=WIN, hop=HOP, tau_min=tau_min, tau_max=tau_max, cmnd=True)["cmnd"][:, :, 1:]
            want = torch_cmnd(x, WIN, HOP, tau_max)
            err = float(((c - want).abs() / want.abs().clamp(min=1e-6)).max())
            if not err < 1e-3:
                raise RuntimeError(f"mvn_pitch_frames differs from the torch expression by {err:.3e} at {(B, T)}")
            res["max_rel_difference_of_c_from_torch_float32"] = err
            res["torch_intermediate_bytes"] = 4 * B * F * WIN * tau_max
            legs["torch_unfold_broadcast"] = lambda: torch_cmnd(x, WIN, HOP, tau_max)
        hip()
        torch.cuda.synchronize(DEV)
        seen = interleaved(legs, rounds, events_us)
        res.update({k: stats(v) for k, v in seen.items()})
        res["frames"] = B * F
        res["multiply_adds"] = B * F * WIN * tau_max
        res["g_multiply_adds_per_s"] = res["multiply_adds"] / (res["mvn_pitch_frames"]["median"] * 1e-6) / 1e9
        out[f"{B}x{T}"] = res
    return dict(what=f"stream time of one call (win {WIN}, hop {HOP}, lags {tau_min} .. {tau_max}), HIP events around "
                     f"{calls} back-to-back calls, us per call", **out)


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
                        "spectral_distance": lambda: model.spectral_distance(gen, src, lengths=[T] * B),
                        "pitch_distance": lambda: model.pitch_distance(gen, src, lengths=[T] * B)}, rounds, wall_ms)
    res = {k: stats(v) for k, v in seen.items()}
    before = res["score"]["median"] + res["spectral_distance"]["median"]
    return dict(what="config 2 under --use_mel, one logged batch of 16 clips x 16000 samples: the WaveNet.score and "
                     "WaveNet.spectral_distance calls of score_samples and the WaveNet.pitch_distance call --score_pitch 1 "
                     "adds (two mvn_pitch_frames launches, the frame span, mvn_pitch_distance), wall ms with a synchronise",
                **res, added_share_of_score_and_distance=res["pitch_distance"]["median"] / before)


def main() -> None:
    rounds, calls = arg("--rounds", 7, int), arg("--calls", 20, int)
    out_path = arg("--out", os.path.join(ROOT, "profiles", "pitch.json"))
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
