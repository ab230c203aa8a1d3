"""The windowed by-rate front end against the by-rate one it stands beside, on 1 x MI355X.

    python scripts/bench_window_frontend.py [--reps 30] [--out profiles/window_frontend.json]

One batch of 16 rows x 160 000 samples at 16 kHz from 44.1 kHz stereo sources, PCM already on the device:

* window: mvn_audio_frontend_window forming 16 windows of 160 000 outputs, each at a drawn out_first of a five-minute
  file (13 230 000 frames), from the spans those windows need (about 441 000 frames each);
* var:    mvn_audio_frontend_var forming the same number of outputs from 16 whole clips of 441 000 frames (10 s).

The two calls alternate in one process (the order rotates every round), HIP events around each, medians reported with
the best and worst round.  Beside them: the bytes the window call's spans upload against what uploading the sixteen
whole files would take.  No target is fixed; both numbers are recorded.  Writes profiles/window_frontend.json."""
import argparse
import json
import os
import random
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from movenet_amd import _native as N  # noqa: E402
from movenet_amd.dataset import WavFolderLoader, resampled_frames  # noqa: E402
from movenet_amd.ops import audio_clip_var_descriptors, audio_clip_window_descriptors  # noqa: E402

DEV = "cuda:0"
B, Q, WIDTH, RATE, AUDIO_RATE, CH = 16, 256, 160000, 44100, 16000, 2
FILE_FRAMES = 5 * 60 * RATE


def timed(legs: dict, reps: int, warmup: int = 3) -> dict:
    """legs: name -> call.  Round r runs the legs rotated by r; returns per-leg statistics in us."""
    names = list(legs)
    times = {k: [] for k in names}
    for r in range(warmup + reps):
        for k in names[r % len(names):] + names[:r % len(names)]:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            legs[k]()
            b.record()
            b.synchronize()
            if r >= warmup:
                times[k].append(a.elapsed_time(b) * 1e3)
    return {k: dict(median_us=statistics.median(v), best_us=min(v), worst_us=max(v), reps=len(v))
            for k, v in times.items()}


def tones(frames: int, seed: int) -> np.ndarray:
    t = np.arange(frames, dtype=np.float64) / RATE
    x = np.stack([0.5 * np.sin(2 * np.pi * (110.0 + 9 * seed + 3 * c) * t) + 0.3 * np.sin(2 * np.pi * 523.3 * t + seed)
                  for c in range(CH)], axis=1)
    return np.round(x * 32767.0).astype(np.int16)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join("profiles", "window_frontend.json"))
    args = ap.parse_args()
    lib, rng = N.lib(), random.Random(7)
    n_file = resampled_frames(FILE_FRAMES, RATE, AUDIO_RATE)
    starts = [rng.randint(0, n_file - WIDTH) for _ in range(B)]
    plans = [WavFolderLoader.window_plan(FILE_FRAMES, RATE, WIDTH, AUDIO_RATE, o) for o in starts]
    with torch.cuda.device(DEV):
        stream = torch.cuda.current_stream(DEV).cuda_stream
        spans = torch.from_numpy(np.concatenate([tones(p[1], b).reshape(-1) for b, p in enumerate(plans)])).to(DEV)
        win = torch.from_numpy(audio_clip_window_descriptors(
            [p[0] for p in plans], [p[1] for p in plans], [FILE_FRAMES] * B, [CH] * B, starts, [p[2] for p in plans],
            [RATE] * B, AUDIO_RATE)).to(DEV)
        clip_frames = WIDTH * 441 // 160
        clips = torch.from_numpy(np.concatenate([tones(clip_frames, b).reshape(-1) for b in range(B)])).to(DEV)
        var = torch.from_numpy(audio_clip_var_descriptors([clip_frames] * B, [CH] * B, [WIDTH] * B)).to(DEV)
        y = torch.empty(B, WIDTH, dtype=torch.float32, device=DEV)
        idx = torch.empty(B, WIDTH, dtype=torch.int32, device=DEV)
        scratch = torch.empty(max(int(lib.mvn_audio_frontend_window_scratch_floats(B, WIDTH)), 2), dtype=torch.float32,
                              device=DEV)
        legs = {
            "window": lambda: N.check(lib.mvn_audio_frontend_window(
                spans.data_ptr(), spans.numel(), win.data_ptr(), B, Q, WIDTH, 1, y.data_ptr(), scratch.data_ptr(),
                idx.data_ptr(), stream), "mvn_audio_frontend_window"),
            "var": lambda: N.check(lib.mvn_audio_frontend_var(
                clips.data_ptr(), clips.numel(), var.data_ptr(), B, Q, WIDTH, 1, y.data_ptr(), scratch.data_ptr(),
                idx.data_ptr(), stream), "mvn_audio_frontend_var"),
        }
        legs["window"]()
        torch.cuda.synchronize(DEV)
        assert int(idx.min()) >= 0, "a window was refused on the device"
        result = dict(
            workload=f"{B} rows x {WIDTH} outputs at {AUDIO_RATE} Hz from {RATE} Hz {CH}-channel PCM on the device; "
                     f"window: out_first drawn in files of {FILE_FRAMES} frames; var: whole clips of {clip_frames} frames",
            device=torch.cuda.get_device_name(DEV), stream_time=timed(legs, args.reps),
            window_upload_bytes=int(spans.numel()) * 2, whole_file_upload_bytes=B * FILE_FRAMES * CH * 2,
            var_upload_bytes=int(clips.numel()) * 2)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
