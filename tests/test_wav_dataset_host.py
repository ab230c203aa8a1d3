"""CPU: the WAV-folder source -- layout, skip rules, sharding, refusals -- and the float64 restatement of the
front end's arithmetic (tests/wav_material.py) against closed forms.  Nothing here needs a GPU: the loader is
constructed and its order inspected, never iterated (iteration launches HIP kernels)."""
import math
import os

import numpy as np
import pytest

import wav_material as M
from movenet_amd.dataset import (SyntheticLoader, WavFolderLoader, get_dataloader, read_wav_header,
                                 read_wav_pcm16)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("wavs")
    return root, M.write_tree(root)


# ---- the restatement against closed forms -------------------------------------------------------------------------

@pytest.mark.parametrize("n,n_out,f", [(4000, 4000, 0.02), (3000, 4000, 0.03), (4410, 1600, 0.01),
                                       (4001, 1600, 0.012)])
def test_sine_comes_back_as_the_same_sine(n, n_out, f):
    """A sine of f cycles per input sample, well below both Nyquist limits, resampled from n to n_out frames is the
    same sine at positions k orig/new, to the bound the window gives (wav_material.interpolation_error_bound: the
    passband deviation |H(f) - 1| plus every image |H(f + j)|), away from the zero-padded ends.  n == n_out is the
    identity up to the 0.99 roll-off: the same bound with orig = new = 1."""
    m = np.sin(2 * np.pi * f * np.arange(n) + 0.4)
    y = M.resample_np(m, n_out)
    g = math.gcd(n, n_out)
    orig, new = n // g, n_out // g
    c = np.arange(n_out) * orig / new
    reach = 6.0 / (0.99 * min(orig, new) / orig) + 2
    inside = (c > reach) & (c < n - 1 - reach)
    err = np.abs(y - np.sin(2 * np.pi * f * c + 0.4))[inside].max()
    bound = M.interpolation_error_bound(f, n, n_out)
    print(f"n={n} n_out={n_out} f={f}: error {err:.3e}, bound from the window {bound:.3e}")
    assert inside.sum() > n_out // 2
    assert bound < 1e-3      # Hann window of six zero crossings: the response is flat to 1e-3 this far below cutoff
    assert err <= bound
    if n == n_out:           # identity: every input sample itself, to the same bound
        assert np.abs(y - m)[inside].max() <= bound


def test_phase_is_exact_for_long_coprime_clips():
    """k orig is a 64-bit integer product: for a coprime length near 2^31 / N the positions still land on the
    exact phase (a float32 product k * orig / new would be off by whole samples)."""
    n, n_out = 200001, 160000
    k = np.array([159999], dtype=np.int64)
    assert int(k[0]) * n > 2 ** 31
    f = 0.001
    m = np.sin(2 * np.pi * f * np.arange(n))
    y = M.resample_np(m, n_out)
    c = 159000 * n / n_out
    assert abs(y[159000] - math.sin(2 * np.pi * f * c)) <= M.interpolation_error_bound(f, n, n_out)


@pytest.mark.parametrize("Q", [64, 256])
def test_silent_clip_stays_silent_and_maps_to_the_mid_class(Q):
    pcm = np.zeros((4000, 1), dtype=np.int16)
    y, q = M.frontend_np(pcm, 1600, Q, normalize=True)
    assert not y.any()
    assert (q == Q // 2).all()      # int((0 + 1) / 2 * (Q - 1) + 0.5)
    assert (M.frontend_np(pcm, 1600, Q, normalize=False)[1] == Q // 2).all()


def test_normalised_clip_spans_every_class_end_to_end():
    pcm = M.as_pcm16(M.quantise(M.signal("sines", 8000, 8000, 1, 0), 2))
    y, q = M.frontend_np(pcm, 16000, 256)
    assert q.min() == 0 and q.max() == 255


def test_fp32_evaluation_of_the_same_formula_stays_close(tree):
    """What the GPU test derives the kernel's tolerance from: float32 numpy against float64 on the material tree,
    Q = 256, N = 160000.  Measured: waveform deviation 3.05e-7 at most (amplitudes ~0.9), class indices differ at
    1.64e-5 of the positions (21 of 1 280 000) and never by more than one class."""
    dev, differ, total = 0.0, 0, 0
    for c in tree[1]:
        y64, q64 = M.frontend_np(c["pcm"], 160000, 256, dtype=np.float64)
        y32, q32 = M.frontend_np(c["pcm"], 160000, 256, dtype=np.float32)
        assert y32.dtype == np.float32
        dev = max(dev, float(np.abs(y32.astype(np.float64) - y64).max()))
        assert np.abs(q32 - q64).max() <= 1
        differ += int((q32 != q64).sum())
        total += q64.size
    print(f"fp32 numpy vs float64: waveform deviation {dev:.3e}, indices differ at {differ}/{total} = {differ / total:.3e}")
    assert dev < 1e-6               # a few ulp of amplitudes below 1
    assert differ / total < 1e-4    # comfortably small: the samples do not sit on class boundaries


# ---- layout, skip rules, info ---------------------------------------------------------------------------------------

def test_layout_contexts_filepaths_info(tree):
    root, clips = tree
    ld = WavFolderLoader(root, 256, batch_size=3)
    assert ld.contexts == ["music", "speech"]
    assert ld.filepaths == [c["path"] for c in clips]
    assert not any("_raw" in os.path.basename(p) or os.path.basename(p).startswith(".") for p in ld.filepaths)
    on_disk = {f for ctx in ld.contexts for f in os.listdir(os.path.join(root, "train", ctx))}
    assert {s + ".wav" for s in M.SKIPPED} <= on_disk          # the skipped files ARE on disk
    for info, c in zip(ld.info, clips):
        assert info == dict(video_fps=0.0, audio_fps=float(c["rate"]), video_orig_dim=0, audio_orig_dim=c["frames"])
    assert len(ld) == math.ceil(len(clips) / 3)
    valid = WavFolderLoader(root, 256, batch_size=3, train=False)
    assert valid.n_clips == 2 and all(os.sep + "valid" + os.sep in p for p in valid.filepaths)
    assert math.gcd(max(c["frames"] for c in clips if "coprime" in c["name"]), 160000) == 1


def test_wav_reader_widths(tree, tmp_path):
    root, clips = tree
    for c in clips:
        pcm, n, ch, rate = read_wav_pcm16(c["path"])
        assert (n, ch, rate) == (c["frames"], c["channels"], c["rate"])
        assert np.array_equal(pcm.reshape(n, ch), c["pcm"])
    # 24- and 32-bit: rounded to the nearest 16-bit value
    import wave
    vals = np.array([0, 1 << 15, -(1 << 15), (1 << 23) - 1, -(1 << 23), 127, 128, -129], dtype=np.int64)
    for width in (3, 4):
        v = vals << (8 * (width - 3))
        raw = b"".join(int(x).to_bytes(width, "little", signed=True) for x in v)
        p = str(tmp_path / f"w{width}.wav")
        with wave.open(p, "wb") as w:
            w.setnchannels(1), w.setsampwidth(width), w.setframerate(8000), w.writeframes(raw)
        pcm, n, ch, _ = read_wav_pcm16(p)
        assert pcm.tolist() == [0, 128, -128, 32767, -32768, 0, 1, -1]
    assert read_wav_header(clips[0]["path"])["width"] in (1, 2)


# ---- sharding -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world", [1, 2, 3])
def test_sharding_covers_every_clip_and_pads_like_the_synthetic_loader(tree, world):
    root, clips = tree
    n = len(clips)
    assert n % 3 != 0 and n % 2 == 0 and n == 8
    for shuffle in (False, True):
        shards, twins = [], []
        for rank in range(world):
            ld = WavFolderLoader(root, 256, batch_size=2, rank=rank, world_size=world, shuffle=shuffle)
            tw = SyntheticLoader(f"synthetic://clips={n},frames=100,seed=1234", 256, 2, rank=rank,
                                 world_size=world, shuffle=shuffle)
            ld.set_epoch(3), tw.set_epoch(3)
            shards.append(ld._order())
            twins.append(tw._order())
            assert len(ld) == len(tw) == math.ceil(math.ceil(n / world) / 2)
        assert shards == twins                                   # same padding and stride, same seeded shuffle
        assert len({len(s) for s in shards}) == 1                # padded: every rank takes equally many
        assert set().union(*shards) == set(range(n))             # the union covers every clip
        assert sum(len(s) for s in shards) == math.ceil(n / world) * world


def test_shuffle_differs_between_epochs_and_agrees_across_ranks(tree):
    root, _ = tree
    full = []
    for epoch in (0, 1):
        per_rank = []
        for rank in range(2):
            ld = WavFolderLoader(root, 256, batch_size=2, rank=rank, world_size=2, shuffle=True)
            ld.set_epoch(epoch)
            per_rank.append(ld._order())
        one = WavFolderLoader(root, 256, batch_size=2, shuffle=True)
        one.set_epoch(epoch)
        whole = one._order()
        assert per_rank[0] == whole[0::2] and per_rank[1] == whole[1::2]   # the ranks stride ONE permutation
        full.append(whole)
    assert full[0] != full[1] and sorted(full[0]) == sorted(full[1])
    fixed = WavFolderLoader(root, 256, batch_size=2, shuffle=False)
    assert fixed._order() == list(range(8))


# ---- refusals and dispatch ---------------------------------------------------------------------------------------

def test_float_wav_is_refused_by_name(tmp_path):
    d = tmp_path / "train" / "ctx"
    d.mkdir(parents=True)
    M.write_float_wav(str(d / "floaty.wav"))
    with pytest.raises(ValueError, match="floaty.wav"):
        WavFolderLoader(tmp_path, 256, batch_size=1)
    with pytest.raises(ValueError, match="floaty.wav"):
        read_wav_pcm16(str(d / "floaty.wav"))


def test_video_refusals(tmp_path, monkeypatch):
    import movenet_amd.wavenet as W
    M.write_tree(tmp_path, material=M.MATERIAL[:2], valid=1, skipped=False)
    with pytest.raises(ValueError, match=r"\.npy"):                       # no frames beside the clip
        WavFolderLoader(tmp_path, 256, batch_size=1, use_video=True)
    with pytest.raises(ValueError, match="batch_subsample_frac"):        # a video request with a crop
        WavFolderLoader(tmp_path, 256, batch_size=1, use_video=True, batch_subsample_frac=0.5)
    monkeypatch.setattr(W, "MAX_AUDIO_FRAMES", 2500)
    with pytest.raises(ValueError, match="1000"):
        WavFolderLoader(tmp_path, 256, batch_size=1, use_video=True)
    # with the frames present the loader is built, and subsamples by linspace / clamp / truncate
    monkeypatch.setattr(W, "MAX_AUDIO_FRAMES", 3000)
    frames = np.arange(7, dtype=np.float32)[:, None, None] * np.ones((1, 64, 64), np.float32) / 10
    for fp in [c["path"] for c in M.write_tree(tmp_path, material=M.MATERIAL[:2], valid=1, skipped=False)]:
        np.save(fp[:-4] + ".npy", frames[..., None] if "8k" in fp else frames)
    ld = WavFolderLoader(tmp_path, 256, batch_size=1, use_video=True)
    v = ld._video(0)
    assert v.shape == (3, 64, 64, 1) and v.dtype == np.float32
    assert np.allclose(v[:, 0, 0, 0], [0.0, 0.3, 0.6])                  # linspace(0, 6, 3) = 0, 3, 6


def test_empty_split_is_refused(tmp_path):
    (tmp_path / "train" / "ctx").mkdir(parents=True)
    with pytest.raises(ValueError, match="no .wav clips"):
        WavFolderLoader(tmp_path, 256, batch_size=1)
    M.write_tree(tmp_path, material=M.MATERIAL[:1], valid=0, skipped=False)
    WavFolderLoader(tmp_path, 256, batch_size=1)
    with pytest.raises(ValueError, match="valid"):                       # train exists, valid does not
        WavFolderLoader(tmp_path, 256, batch_size=1, train=False)


def test_dispatch(tree):
    root, clips = tree
    ld = get_dataloader(str(root), 64, batch_size=2, use_video=False, batch_subsample_frac=0.25, shuffle=True,
                        num_workers=3, pin_memory=True, world_size=0)
    assert isinstance(ld, WavFolderLoader) and ld.frac == 0.25 and ld.shuffle and ld.Q == 64
    assert ld.cache_stats() == dict(hits=0, misses=0, clips=0, bytes=0)
    assert isinstance(get_dataloader("synthetic://clips=2,frames=100", 64, use_video=False), SyntheticLoader)
    with pytest.raises(ValueError):
        get_dataloader("/data/kinetics", 64)
    with pytest.raises(ValueError):                                      # a directory without train/ or valid/
        get_dataloader(os.path.join(str(root), "train"), 64)


def test_iterating_without_a_gpu_is_an_error_not_a_fallback(tree):
    ld = WavFolderLoader(tree[0], 256, batch_size=2)
    with pytest.raises(RuntimeError, match="HIP"):
        next(iter(ld))
