"""The loader's video front end on 1 x MI355X: one batch of 8 clips x 32 selected frames of 256 x 340 RGB (config 3's
clip) -> (8, 32, 64, 64) uint8 levels, under both antialias settings.
(a) the launch as stream time per launch, in a burst of launches between two HIP events, with the bytes it has to read
    (every source row with antialias; the two rows per output row without) against the HBM peak;
(b) the same work in torch on 16 host threads: the oracle's expression (rgb_to_grayscale restated, interpolate, round);
(c) a config-3 Trainer.fit (30 layers, C = K = 64, 8 clips of 32 frames, T = 32000) over a small raw-frame folder: the
    first epoch (every clip a miss: file read, upload, launch) against the following ones (every clip a cache hit),
    after a warm-up fit on a copy of the folder.
Writes profiles/video_frontend.json.
Usage: python scripts/bench_video_frontend.py [--out PATH]"""
import json
import os
import shutil
import sys
import tempfile
import time
import wave

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import movenet_amd.wavenet as W  # noqa: E402
from movenet_amd.ops import video_frontend  # noqa: E402

DEV = torch.device("cuda:0")
B, N, H, WID, FILE_FRAMES, CLIPS = 8, 32, 256, 340, 40, 16
HBM_PEAK_TBS = 8.0
BURST = 20


def burst_ms(fn, reps: int = 5) -> list:
    for _ in range(3):
        fn()
    torch.cuda.synchronize(DEV)
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(BURST):
            fn()
        b.record()
        torch.cuda.synchronize(DEV)
        out.append(a.elapsed_time(b) / BURST)
    return out


def rows_read(h: int, antialias: bool) -> int:
    """Source rows one frame's 64 output rows need."""
    if antialias:
        return h
    rows = set()
    for i in range(64):
        y = min(int(max(h / 64.0 * (i + 0.5) - 0.5, 0.0)), h - 1)
        rows.update((y, min(y + 1, h - 1)))
    return len(rows)


def torch_cpu(frames: torch.Tensor, antialias: bool) -> torch.Tensor:
    r, g, b = frames[..., 0], frames[..., 1], frames[..., 2]
    l = (0.2989 * r + 0.587 * g + 0.114 * b).to(torch.uint8)
    y = torch.nn.functional.interpolate(l.float()[:, None], size=(64, 64), mode="bilinear", align_corners=False,
                                        antialias=antialias)
    return torch.round(y).to(torch.uint8)[:, 0]


def write_folder(root: str, rng) -> None:
    for split, count in (("train", CLIPS), ("valid", 1)):
        d = os.path.join(root, split, "dance")
        os.makedirs(d)
        t = np.arange(32000, dtype=np.float64) / 8000.0
        for j in range(count):
            x = 0.6 * np.sin(2 * np.pi * (110.0 + 7 * j) * t) + 0.3 * np.sin(2 * np.pi * 331.0 * t + j)
            with wave.open(os.path.join(d, f"clip{j:02d}.wav"), "wb") as w:
                w.setnchannels(1), w.setsampwidth(2), w.setframerate(8000)
                w.writeframes(np.round(x * 32767.0).astype("<i2").tobytes())
            np.save(os.path.join(d, f"clip{j:02d}.npy"),
                    rng.integers(0, 256, size=(FILE_FRAMES, H, WID, 3), dtype=np.uint8))


def fit_epochs(root: str, out_dir: str, epochs: int):
    from movenet_amd.config import ModelConfig, TrainingConfig
    from movenet_amd.dataset import WavFolderLoader
    from movenet_amd.pytorch_lightning_trainer import Dance2Music, Trainer
    mc = ModelConfig(layer_size=10, stack_size=3, input_channels=256, residual_channels=64, skip_channels=64)
    cfg = TrainingConfig(model_config=mc, batch_size=B, val_batch_size=1, n_epochs=epochs, use_video=True,
                         optimizer="AdamW", learning_rate=1e-4, scheduler=None, model_output_path=out_dir)
    m = Dance2Music(root, cfg)
    tr = Trainer(max_epochs=epochs, default_root_dir=None, gradient_clip_val=0.0, limit_val_batches=1,
                 enable_checkpointing=False)
    t0 = time.perf_counter()
    tr.fit(m)
    torch.cuda.synchronize(DEV)
    total = time.perf_counter() - t0
    stats = WavFolderLoader(root, 256, batch_size=B, use_video=True, device=DEV).cache_stats()
    return [round(s, 4) for s in tr.epoch_seconds], total, stats, len(tr.history)


def main() -> None:
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(
        ROOT, "profiles", "video_frontend.json")
    rng = np.random.default_rng(7)
    frames = rng.integers(0, 256, size=(B * N, H, WID, 3), dtype=np.uint8)
    res = dict(workload=f"{B} clips x {N} selected frames of {H} x {WID} RGB -> ({B}, {N}, 64, 64) uint8 levels",
               device=torch.cuda.get_device_name(DEV), upload_megabytes=frames.size / 1e6, launches_per_burst=BURST)
    torch.set_num_threads(16)
    with torch.cuda.device(DEV):
        pix = torch.from_numpy(frames.reshape(-1)).to(DEV)
        shapes = [(H, WID, 3)] * B
        for aa in (False, True):
            out = torch.empty(B, N, 64, 64, dtype=torch.uint8, device=DEV)
            ms = burst_ms(lambda: video_frontend(pix, shapes, N, antialias=aa, out=out, check=False))
            nbytes = B * N * rows_read(H, aa) * WID * 3
            t0 = time.perf_counter()
            want = torch_cpu(torch.from_numpy(frames), aa)
            cpu_s = [time.perf_counter() - t0]
            for _ in range(2):
                t0 = time.perf_counter()
                torch_cpu(torch.from_numpy(frames), aa)
                cpu_s.append(time.perf_counter() - t0)
            differ = int((out.cpu().reshape(B * N, 64, 64) != want).sum())
            med = sorted(ms)[len(ms) // 2]
            res["antialias_%d" % aa] = dict(
                launch_ms=dict(median=med, all=[round(x, 4) for x in ms]),
                bytes_read=nbytes, read_TB_per_s=nbytes / (med * 1e-3) / 1e12,
                fraction_of_hbm_peak=nbytes / (med * 1e-3) / 1e12 / HBM_PEAK_TBS, hbm_peak_TB_per_s=HBM_PEAK_TBS,
                torch_cpu_16_threads_ms=dict(best=min(cpu_s) * 1e3, all=[round(s * 1e3, 2) for s in cpu_s]),
                cpu_over_gpu=min(cpu_s) * 1e3 / med,
                levels_differing_from_torch_fp32=differ, levels=B * N * 64 * 64)
    W.MAX_VIDEO_FRAMES, W.MAX_AUDIO_FRAMES = N, 1000 * N
    with tempfile.TemporaryDirectory() as tmp:
        a, b = os.path.join(tmp, "warm"), os.path.join(tmp, "data")
        write_folder(a, rng)
        shutil.copytree(a, b)
        fit_epochs(a, os.path.join(tmp, "out"), 1)          # code objects, allocator, pinned buffers
        epochs, total, stats, steps = fit_epochs(b, os.path.join(tmp, "out"), 3)
        res["trainer_fit_config3"] = dict(
            folder=f"{CLIPS} clips of {FILE_FRAMES} raw {H} x {WID} RGB frames, batch {B}: {steps // 3} steps an epoch",
            epoch_seconds=epochs, first_epoch_misses_s=epochs[0], later_epochs_hits_s=epochs[1:],
            fit_wall_s=total, cache_stats=stats,
            note="wall time of each epoch's training loop (host enqueue; the GPU runs behind it); epoch 0 reads the "
                 "files, uploads and launches, the later ones take every clip from the device cache")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
