"""The loader's waveform front end against the train step it feeds, on 1 x MI355X: 16 stereo 44.1 kHz clips of 10 s
(441 000 frames each) -> 16 x 160 000 class indices -> the (16, 256, 16000) one-hot crop of a config-2 step.
HIP events around (a) the two front-end kernels on PCM already on the device, (b) a whole uncached loader batch
(upload, front end, crop, one-hot), (c) a cached one (int16 rows -> one-hot), and (d) one config-2 train step
(BASELINE configs[1]: 30 layers, C = K = 64, 16 x 16000) in the same process.  The requirement is relative:
(b) < (d), otherwise the loader would gate Trainer.fit.  Writes profiles/audio_frontend.json.
Usage: python scripts/bench_audio_frontend.py [--out PATH]"""
import json
import os
import sys
import tempfile
import time
import wave

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from movenet_amd.dataset import WavFolderLoader, read_wav_pcm16  # noqa: E402
from movenet_amd.ops import audio_frontend  # noqa: E402
from movenet_amd.optim import FlatAdamW, order_like_backward  # noqa: E402
from movenet_amd.utils.weights import make_state_dict, one_hot, synthetic_indices  # noqa: E402
from movenet_amd.wavenet import WaveNet  # noqa: E402

DEV = torch.device("cuda:0")
B, Q, RATE, SECONDS, T_STEP = 16, 256, 44100, 10, 16000
CFG = dict(layer_size=10, stack_size=3, input_channels=Q, residual_channels=64, skip_channels=64)


def write_clips(root: str) -> None:
    d = os.path.join(root, "train", "tones")
    os.makedirs(d)
    t = np.arange(RATE * SECONDS, dtype=np.float64) / RATE
    for j in range(B):
        x = np.stack([0.5 * np.sin(2 * np.pi * (110.0 + 9 * j + 3 * c) * t) + 0.3 * np.sin(2 * np.pi * 523.3 * t + j)
                      for c in range(2)], axis=1)
        with wave.open(os.path.join(d, f"clip{j:02d}.wav"), "wb") as w:
            w.setnchannels(2), w.setsampwidth(2), w.setframerate(RATE)
            w.writeframes(np.round(x * 32767.0).astype("<i2").tobytes())


def gpu_ms(fn, reps: int, warm: int = 2) -> list:
    for _ in range(warm):
        fn()
    torch.cuda.synchronize(DEV)
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    marks[0].record()
    for i in range(reps):
        fn()
        marks[i + 1].record()
    torch.cuda.synchronize(DEV)
    return [marks[i].elapsed_time(marks[i + 1]) for i in range(reps)]


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main() -> None:
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(
        ROOT, "profiles", "audio_frontend.json")
    res = dict(workload=f"{B} stereo {RATE} Hz clips of {SECONDS} s -> {B} x 160000 indices, Q = {Q}; "
                        f"one-hot crop (16, 256, {T_STEP})", device=torch.cuda.get_device_name(DEV))
    with tempfile.TemporaryDirectory() as root, torch.cuda.device(DEV):
        write_clips(root)
        files = sorted(os.listdir(os.path.join(root, "train", "tones")))
        clips = [read_wav_pcm16(os.path.join(root, "train", "tones", f)) for f in files]
        pcm = torch.from_numpy(np.concatenate([c[0] for c in clips])).to(DEV)
        frames, channels = [c[1] for c in clips], [c[2] for c in clips]
        ms = gpu_ms(lambda: audio_frontend(pcm, frames, channels, Q), reps=10)
        res["frontend_kernels_ms"] = dict(median=median(ms), all=[round(x, 4) for x in ms])
        pinned = pcm.cpu().pin_memory()
        ms = gpu_ms(lambda: audio_frontend(pinned.to(DEV, non_blocking=True), frames, channels, Q), reps=10)
        res["upload_and_kernels_ms"] = dict(median=median(ms), all=[round(x, 4) for x in ms],
                                            upload_megabytes=pinned.numel() * 2 / 1e6)

        def loader_batch(cache_bytes):
            ld = WavFolderLoader(root, Q, batch_size=B, batch_subsample_frac=T_STEP / 160000, device=DEV,
                                 cache_bytes=cache_bytes)
            t0 = time.perf_counter()
            batch = next(iter(ld))
            return batch, time.perf_counter() - t0

        host = []
        ms = gpu_ms(lambda: host.append(loader_batch(0)[1]), reps=5, warm=1)   # a cap of 0: every batch is uncached
        res["loader_batch_uncached_ms"] = dict(gpu_median=median(ms), gpu_all=[round(x, 3) for x in ms],
                                               host_enqueue_median=median(host) * 1e3,
                                               note="GPU span between stream events: includes waiting for the "
                                                    "host's file reads and staging when those are slower")
        loader_batch(4 << 30)                                                   # fills the cache
        host = []
        ms = gpu_ms(lambda: host.append(loader_batch(4 << 30)[1]), reps=10)
        res["loader_batch_cached_ms"] = dict(gpu_median=median(ms), gpu_all=[round(x, 3) for x in ms],
                                             host_enqueue_median=median(host) * 1e3)

        model = WaveNet(**CFG)
        model.load_state_dict(make_state_dict(**CFG, seed=0))
        model.to(DEV).train()
        opt = FlatAdamW(order_like_backward(model, with_context=False), lr=1e-4)
        audio = one_hot(synthetic_indices(B, T_STEP, Q, 1234).to(DEV), Q)
        target = audio[:, :, model.receptive_fields:].argmax(1)

        def step():
            opt.zero_grad(set_to_none=True)
            loss, _, _ = model(audio, None, return_loss=True, target=target)
            loss.backward()
            opt.step()

        ms = gpu_ms(step, reps=6, warm=5)
        res["config2_train_step_ms"] = dict(median=median(ms), all=[round(x, 3) for x in ms])
    # the front end of an uncached batch on the GPU: upload + the two kernels + what a cached batch costs as well
    # (gather, crop, one-hot).  The whole-loader figure above also contains the host's file reads (first epoch only).
    step_ms = res["config2_train_step_ms"]["median"]
    uncached = res["upload_and_kernels_ms"]["median"] + res["loader_batch_cached_ms"]["gpu_median"]
    res["uncached_front_end_ms"] = uncached
    res["uncached_front_end_over_train_step"] = uncached / step_ms
    res["uncached_loader_batch_over_train_step"] = res["loader_batch_uncached_ms"]["gpu_median"] / step_ms
    res["requirement_met"] = uncached < step_ms
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
