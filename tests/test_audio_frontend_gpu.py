"""GPU: the waveform front end (mvn_audio_frontend), the WAV-folder loader on the device, and the first test in which
training has to LEARN.

Front end against the float64 restatement (tests/wav_material.py), every clip of the material tree (mono / stereo,
8- / 16-bit, 8 000 - 48 000 Hz, a length coprime to 160 000, a chirp, a silent clip), Q = 256, N = 160 000:

* waveform before quantisation: the kernel may deviate 4 x what a float32 numpy evaluation of the same formula
  deviates from float64 on the same material (the margin covers sinpif / cospif against libm and another summation
  order).  Measured on the CPU: float32 numpy deviates 3.05e-7 at most, so the kernel's tolerance is 1.22e-6
  (the test recomputes both from the material it is given and prints them).  Measured on an MI355X: 3.53e-7.
* class indices: |kernel - float64| <= 1 everywhere; the share of positions that differ at all is at most twice the
  share float32 numpy shows (measured: 21 of 1 280 000 = 1.64e-5, so at most 3.28e-5 for the kernel).  Measured on
  an MI355X: 19 positions, 1.48e-5, never by more than one class.

Learning test.  The trainer's loss is cross_entropy applied to PROBABILITIES (the reference's, kept): it is ln Q for
a uniform output and cannot fall below ln(e + Q - 1) - 1 for a perfect one -- 3.185 against ln 64 = 4.159.  "Below
half of ln Q" is therefore out of reach of ANY model, and no CPU-affordable setting gets the oracle there either:
the torch restatement (oracle/wavenet_oracle.py) with torch's AdamW, lr 3e-3, 400 steps of 2 clips x 4000 frames on
the same four two-sine clips, ended at loss 3.648 (mean of the last 10 %), accuracy 0.538.  So the assertion on the
loss is the relative one: final loss <= 1.25 x the oracle's 3.648.  That alone would also pass at ln Q, so a second
bound is held with it: the loss must have covered a quarter of the distance from ln Q to the floor (<= 3.916; the
oracle covers 52 % of it, noise none).  The accuracy bound stays absolute: > 10 / Q (oracle: 0.538 > 15 / Q).  The
control -- the same model, optimizer and number of steps on synthetic:// noise -- stays within 5 % of ln Q.
Measured on an MI355X: waveforms 3.740 / accuracy 0.444 after 400 steps in 3.7 s (first step 4.159); noise 4.159 /
0.016 in 1.6 s.
"""
import math
import os
import time

import numpy as np
import pytest
import torch

import wav_material as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_OUT, Q = 160000, 256
BAND, SENTINEL_F, SENTINEL_I = 1 << 16, -1234.5, -77


@pytest.fixture(scope="module")
def material(tmp_path_factory):
    root = tmp_path_factory.mktemp("wavs")
    clips = M.write_tree(root)
    ref = []
    for c in clips:
        y64, q64 = M.frontend_np(c["pcm"], N_OUT, Q, dtype=np.float64)
        y32, q32 = M.frontend_np(c["pcm"], N_OUT, Q, dtype=np.float32)
        ref.append(dict(y64=y64, q64=q64, y32=y32, q32=q32))
    return root, clips, ref


def _run_frontend(clips, normalize=True, q=Q):
    """All clips in one call, outputs carved out of sentinel-filled buffers; returns (idx, y, band check)."""
    from movenet_amd.ops import audio_frontend
    B = len(clips)
    pcm = torch.from_numpy(np.concatenate([c["pcm"].reshape(-1) for c in clips])).to(DEV)
    raw_i = torch.full((B * N_OUT + BAND,), SENTINEL_I, dtype=torch.int32, device=DEV)
    raw_y = torch.full((B * N_OUT + BAND,), SENTINEL_F, dtype=torch.float32, device=DEV)
    idx, y = audio_frontend(pcm, [c["frames"] for c in clips], [c["channels"] for c in clips], q, n_out=N_OUT,
                            normalize=normalize, return_waveform=True, out=raw_i[:B * N_OUT].view(B, N_OUT),
                            waveform_out=raw_y[:B * N_OUT].view(B, N_OUT))
    torch.cuda.synchronize()
    untouched = bool((raw_i[B * N_OUT:] == SENTINEL_I).all()) and bool((raw_y[B * N_OUT:] == SENTINEL_F).all())
    return idx, y, untouched


def test_frontend_matches_float64_restatement(material):
    _, clips, ref = material
    idx, y, untouched = _run_frontend(clips)
    assert untouched, "mvn_audio_frontend wrote behind its (B, N) outputs"
    idx, y = idx.cpu().numpy().astype(np.int64), y.cpu().numpy().astype(np.float64)
    fp32_dev = max(float(np.abs(r["y32"].astype(np.float64) - r["y64"]).max()) for r in ref)
    fp32_differ = sum(int((r["q32"] != r["q64"]).sum()) for r in ref)
    total = len(ref) * N_OUT
    tol, cap = 4.0 * fp32_dev, 2.0 * fp32_differ / total
    assert 0 < fp32_dev < 1e-6 and fp32_differ / total < 1e-4     # the condition the cap rests on (also a CPU test)
    differ = 0
    for b, (c, r) in enumerate(zip(clips, ref)):
        dev = float(np.abs(y[b] - r["y64"]).max())
        dq = np.abs(idx[b] - r["q64"])
        differ += int((dq != 0).sum())
        print(f"{c['name']}: waveform deviation {dev:.3e} (tolerance {tol:.3e}), indices differ at "
              f"{int((dq != 0).sum())} positions, by {int(dq.max())} at most")
        assert dev <= tol, (c["name"], dev, tol)
        assert dq.max() <= 1, c["name"]
    print(f"fp32 numpy: deviation {fp32_dev:.3e}, differing share {fp32_differ / total:.3e}; "
          f"kernel: differing share {differ / total:.3e} (cap {cap:.3e})")
    assert differ / total <= cap
    silent = [b for b, c in enumerate(clips) if "silence" in c["name"]]
    assert silent and all((idx[b] == Q // 2).all() and not y[b].any() for b in silent)


def test_frontend_is_bit_reproducible_and_batch_independent(material):
    _, clips, _ = material
    a, ya, _ = _run_frontend(clips)
    b, yb, _ = _run_frontend(clips)
    assert torch.equal(a, b) and torch.equal(ya, yb)
    # a clip alone, behind other clips in the upload, or in another row gives the same bits
    one, y1, ok = _run_frontend(clips[3:4])
    assert ok and torch.equal(one[0], a[3]) and torch.equal(y1[0], ya[3])


def test_frontend_without_normalisation_and_other_class_counts(material):
    _, clips, _ = material
    sub = clips[:3]
    for q, normalize in ((64, True), (256, False)):
        idx, y, ok = _run_frontend(sub, normalize=normalize, q=q)
        assert ok
        for b, c in enumerate(sub):
            want = M.quantise_np(M.resample_np(M.downmix_np(c["pcm"]), N_OUT), q, normalize)
            dq = np.abs(idx[b].cpu().numpy().astype(np.int64) - want)
            assert dq.max() <= 1 and (dq != 0).mean() < 1e-3, (c["name"], q, normalize)


def test_descriptor_outside_the_upload_is_refused_on_the_device(material):
    """The descriptors are device data: a span that does not lie inside the upload is never read through, and its
    row is filled with -1 (the other rows are computed as usual)."""
    from movenet_amd.ops import audio_clip_descriptors, audio_frontend
    _, clips, _ = material
    sub = clips[:2]
    pcm = torch.from_numpy(np.concatenate([c["pcm"].reshape(-1) for c in sub])).to(DEV)
    frames, channels = [c["frames"] for c in sub], [c["channels"] for c in sub]
    good = audio_frontend(pcm, frames, channels, Q, n_out=N_OUT)
    desc = audio_clip_descriptors(frames, channels)
    rec = desc.view([("offset", "<i8"), ("frames", "<i4"), ("channels", "<i4")]).reshape(2)
    rec["offset"][1] = pcm.numel() - 10          # 10 samples left, `frames` claimed
    bad = audio_frontend(pcm, frames, channels, Q, n_out=N_OUT, descriptors=torch.from_numpy(desc).to(DEV))
    assert torch.equal(bad[0], good[0]) and bool((bad[1] == -1).all())
    with pytest.raises(ValueError, match="do not lie inside"):   # host lists are checked before any launch
        audio_frontend(pcm, frames, channels, Q, n_out=N_OUT, offsets=[0, pcm.numel() - 10])
    with pytest.raises(ValueError, match="100 x"):
        audio_frontend(pcm[:20000], [20000], [1], Q, n_out=100)


# ---- the loader on the device ------------------------------------------------------------------------------------

def test_loader_batches_cache_and_crop(material):
    from movenet_amd.dataset import get_dataloader
    root, clips, ref = material
    ld = get_dataloader(str(root), Q, batch_size=3, use_video=False, device=DEV)
    first = []
    for batch in ld:
        a = batch.audio
        B = a.shape[0]
        assert tuple(a.shape) == (B, Q, N_OUT) and a.dtype == torch.float32 and a.is_cuda
        assert bool(((a == 0) | (a == 1)).all()) and bool((a.sum(1) == 1).all())    # every column exactly one-hot
        assert batch.video is None and len(batch.contexts) == len(batch.filepaths) == len(batch.info) == B
        first.append(batch)
    assert [fp for b in first for fp in b.filepaths] == [c["path"] for c in clips]
    assert [c for b in first for c in b.contexts] == [c["context"] for c in clips]
    got = torch.cat([b.audio.argmax(1) for b in first]).cpu().numpy()
    assert all(np.abs(got[i] - ref[i]["q64"]).max() <= 1 for i in range(len(clips)))
    assert ld.cache_stats()["hits"] == 0 and ld.cache_stats()["misses"] == len(clips)
    assert ld.cache_stats()["bytes"] == len(clips) * N_OUT * 2
    # second epoch (a NEW loader, as the trainer builds one per epoch): every clip is a hit, same batches
    ld2 = get_dataloader(str(root), Q, batch_size=3, use_video=False, device=DEV)
    ld2.set_epoch(1)
    for b1, b2 in zip(first, ld2):
        assert torch.equal(b1.audio, b2.audio) and b1.filepaths == b2.filepaths
    assert ld2.cache_stats()["hits"] == len(clips) and ld2.cache_stats()["misses"] == len(clips)
    del first
    # the crop of dataset.py:232-237: ceil(T * frac) frames, one start per batch, a window of the full batch
    frac = 0.3
    ld3 = get_dataloader(str(root), Q, batch_size=4, use_video=False, device=DEV, batch_subsample_frac=frac)
    batch = next(iter(ld3))
    n = math.ceil(N_OUT * frac)
    assert tuple(batch.audio.shape) == (4, Q, n) and bool((batch.audio.sum(1) == 1).all())
    crop = batch.audio.argmax(1).cpu().numpy()
    starts = [s for s in range(N_OUT - n + 1) if np.array_equal(got[0, s:s + 8], crop[0, :8])]
    assert any(np.array_equal(got[:4, s:s + n], crop) for s in starts)
    # a cap too small for a clip: nothing is cached, nothing evicted, every epoch misses
    ld4 = get_dataloader(str(root), Q, batch_size=4, use_video=False, device=DEV, cache_bytes=1000)
    for _ in range(2):
        assert sum(b.audio.shape[0] for b in ld4) == len(clips)
    assert ld4.cache_stats() == dict(hits=0, misses=2 * len(clips), clips=0, bytes=0)


def test_loader_video_frames(tmp_path, monkeypatch):
    import movenet_amd.wavenet as W
    from movenet_amd.dataset import WavFolderLoader
    monkeypatch.setattr(W, "MAX_AUDIO_FRAMES", 3000)
    clips = M.write_tree(tmp_path, material=M.MATERIAL[:2], valid=1, skipped=False)
    rng = np.random.default_rng(3)
    vids = []
    for c in clips:
        v = rng.random((7, 64, 64), dtype=np.float32)
        np.save(c["path"][:-4] + ".npy", v)
        vids.append(v[[0, 3, 6]][..., None])
    batch = next(iter(WavFolderLoader(tmp_path, 64, batch_size=2, use_video=True, device=DEV)))
    assert tuple(batch.audio.shape) == (2, 64, 3000) and tuple(batch.video.shape) == (2, 3, 64, 64, 1)
    assert np.array_equal(batch.video.cpu().numpy(), np.stack(vids))


# ---- training learns ------------------------------------------------------------------------------------------------

ORACLE_FINAL_LOSS, ORACLE_FINAL_ACC = 3.648, 0.538     # CPU oracle, same material / model / optimizer / steps
LEARN_Q, STEPS = 64, 400


def _fit(dataset, tmp_path, epochs):
    from movenet_amd.config import ModelConfig, TrainingConfig
    from movenet_amd.pytorch_lightning_trainer import Dance2Music, Trainer
    from movenet_amd.utils.weights import make_state_dict
    mc = ModelConfig(layer_size=4, stack_size=2, input_channels=LEARN_Q, residual_channels=32, skip_channels=32)
    is_dir = os.path.isdir(dataset)
    cfg = TrainingConfig(model_config=mc, batch_size=2, val_batch_size=1, n_epochs=epochs, use_video=False,
                         optimizer="AdamW", learning_rate=3e-3, weight_decay=0.0, scheduler=None,
                         batch_subsample_frac=0.025 if is_dir else None,
                         val_batch_subsample_frac=0.025 if is_dir else None, model_output_path=tmp_path)
    m = Dance2Music(dataset, cfg)
    m.model.load_state_dict(make_state_dict(4, 2, LEARN_Q, 32, 32, seed=11))
    tr = Trainer(max_epochs=epochs, default_root_dir=None, gradient_clip_val=0.0, limit_val_batches=1)
    tr.fit(m)
    assert len(tr.history) == STEPS
    tail = tr.history[-STEPS // 10:]
    return (float(np.mean([h["train_loss"] for h in tail])), float(np.mean([h["train_acc"] for h in tail])),
            tr.history[0]["train_loss"])


def test_training_on_waveforms_learns_and_on_noise_does_not(tmp_path):
    """Four two-sine clips (8 kHz, 2 s, resampled to 160 000 frames), 4 x 2 layers, C = K = 32, Q = 64, AdamW
    3e-3, 400 steps of 2 clips x 4000 frames.  Bounds, the oracle's figures and the measured ones (5.3 s for both
    runs on an MI355X): the module docstring."""
    ln_q, floor = math.log(LEARN_Q), math.log(math.e + LEARN_Q - 1) - 1
    root = tmp_path / "tones"
    M.write_learning_tree(root)
    t0 = time.perf_counter()
    loss, acc, loss0 = _fit(str(root), tmp_path, epochs=STEPS // 2)           # 4 clips / batch 2 = 2 steps an epoch
    t1 = time.perf_counter()
    noise_loss, noise_acc, _ = _fit(f"synthetic://clips={STEPS},frames=4000,seed=3", tmp_path, epochs=2)
    t2 = time.perf_counter()
    print(f"waveforms: first step {loss0:.4f}, last 10 % loss {loss:.4f} acc {acc:.4f} in {t1 - t0:.1f} s "
          f"(oracle {ORACLE_FINAL_LOSS} / {ORACLE_FINAL_ACC}); noise: loss {noise_loss:.4f} acc {noise_acc:.4f} "
          f"in {t2 - t1:.1f} s; ln Q {ln_q:.4f}, floor {floor:.4f}")
    assert abs(loss0 - ln_q) < 0.05 * ln_q                      # it starts where noise stays
    assert loss <= 1.25 * ORACLE_FINAL_LOSS                     # the issue's relative bound
    assert loss <= ln_q - 0.25 * (ln_q - floor)                 # ... and a quarter of the way to the floor
    assert acc > 10.0 / LEARN_Q
    assert abs(noise_loss - ln_q) <= 0.05 * ln_q                # the control: the drop comes from the data
    assert noise_acc < 10.0 / LEARN_Q
