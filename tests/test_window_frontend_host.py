"""CPU: the host side of training on random windows of long recordings (WavFolderLoader(clip_length="window"), DESIGN
4.5e): the span a window needs, window counts and tiling, the training draws, reading a span of a WAV, the new exports
and their host refusals, the flags."""
import ctypes
import math
import os

import numpy as np
import pytest

import wav_material as M
import window_reference as R
from movenet_amd import _native as N

RATES = ((44100, 16000), (8000, 12000), (48000, 16000), (16000, 16000))


def _taps_brute_force(file_frames, rate, audio_rate, out_first, n_out):
    """(first, last) source frame any tap of the columns reaches, clipped to the file: every (j, d) pair written out"""
    orig, new, _, W = R.geometry(rate, audio_rate)
    j = out_first + np.arange(n_out, dtype=np.int64)
    at = (j * orig // new)[:, None] + np.arange(-W, W + 2, dtype=np.int64)[None, :]
    at = at[(at >= 0) & (at < file_frames)]
    return int(at.min()), int(at.max())


@pytest.mark.parametrize("rate,audio_rate", RATES)
def test_window_plan_covers_exactly_the_taps_range(rate, audio_rate):
    from movenet_amd.dataset import WavFolderLoader, resampled_frames, window_geometry
    plan = WavFolderLoader.window_plan
    orig, new, s, W = R.geometry(rate, audio_rate)
    assert window_geometry(rate, audio_rate) == (orig, new, W)
    frames, file_frames = 700, 10 * rate + 123
    n_file = math.ceil(file_frames * new / orig)
    assert resampled_frames(file_frames, rate, audio_rate) == n_file == R.n_file(file_frames, rate, audio_rate)
    for out_first in (0, 1, n_file // 2, n_file - frames, n_file - frames + 1, n_file - 1):
        first, span, n_out = plan(file_frames, rate, frames, audio_rate, out_first)
        assert n_out == min(frames, n_file - out_first) >= 1
        lo, hi = _taps_brute_force(file_frames, rate, audio_rate, out_first, n_out)
        assert (first, first + span - 1) == (lo, hi), (out_first, first, span, lo, hi)
        assert 0 <= first and first + span <= file_frames
    assert plan(file_frames, rate, frames, audio_rate, 0)[0] == 0                      # the file's start
    first, span, _ = plan(file_frames, rate, frames, audio_rate, n_file - frames)
    assert first + span == file_frames                                                 # ... and its end
    for bad in (-1, n_file):
        with pytest.raises(ValueError):
            plan(file_frames, rate, frames, audio_rate, bad)


def test_window_plan_far_into_a_long_file():
    """out_first * orig beyond 2^32: the products are Python integers, and the span stays a window's worth"""
    from movenet_amd.dataset import WavFolderLoader
    rate, audio_rate, frames, out_first = 44100, 16000, 2304, 40_000_000
    file_frames = 120_000_000
    orig, new, _, W = R.geometry(rate, audio_rate)
    assert out_first * orig > 1 << 32
    first, span, n_out = WavFolderLoader.window_plan(file_frames, rate, frames, audio_rate, out_first)
    assert n_out == frames
    assert (first, first + span - 1) == _taps_brute_force(file_frames, rate, audio_rate, out_first, n_out)
    assert first == out_first * 441 // 160 - W == 110_250_000 - W
    assert span == (frames - 1) * 441 // 160 + 2 * W + 2


def _tree(root, clips, split="train"):
    d = os.path.join(str(root), split, "a")
    os.makedirs(d, exist_ok=True)
    for seed, (name, rate, frames, channels) in enumerate(clips):
        M.write_wav(os.path.join(d, name + ".wav"), M.quantise(M.signal("sines", rate, frames, channels, seed), 2), rate)
    return str(root)


CLIPS = [("a_8k", 8000, 1600, 1), ("b_16k", 16000, 4000, 2), ("c_44k", 44100, 30000, 2), ("d_48k", 48000, 24001, 1)]
F = 3000            # the row width; n_file at 16 kHz: 3200, 4000, 10885, 8001 -> 2, 2, 4, 3 windows


def test_window_counts_and_validation_tiling(tmp_path, monkeypatch):
    import movenet_amd.wavenet as W
    from movenet_amd.dataset import WavFolderLoader
    monkeypatch.setattr(W, "MAX_AUDIO_FRAMES", F)
    count = WavFolderLoader.window_count
    assert count(1600, 8000, F, 16000) == 2 and count(100, 8000, F, 16000) == 1
    assert count(6000, 16000, F, 16000) == 2 and count(6001, 16000, F, 16000) == 3
    root = _tree(tmp_path, CLIPS, "valid")
    ld = WavFolderLoader(root, 64, 3, train=False, clip_length="window", audio_rate=16000)
    assert ld.window and not ld.native and ld.frames == F
    assert ld.n_file == [3200, 4000, 10885, 8001]
    assert ld.pairs == [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2), (2, 3), (3, 0), (3, 1), (3, 2)]
    assert len(ld) == math.ceil(11 / 3)
    # validation windows partition [0, n_file): window w starts at w * frames and the last one is short
    for i, n in enumerate(ld.n_file):
        at = 0
        for w in [w for f, w in ld.pairs if f == i]:
            start = ld.window_start(i, w)
            h = ld.index[i][2]
            _, _, n_out = ld.window_plan(h["frames"], h["rate"], F, 16000, start)
            assert start == at == w * F and 1 <= n_out <= F
            at += n_out
        assert at == n
    # the epoch does not move them
    ld.set_epoch(3)
    assert [ld.window_start(i, w) for i, w in ld.pairs] == [w * F for _, w in ld.pairs]
    # a file shorter than the row: one window of n_file samples
    short = WavFolderLoader(_tree(tmp_path / "s", [("s", 8000, 500, 1)], "valid"), 64, 3, train=False,
                            clip_length="window")
    assert short.pairs == [(0, 0)] and short.window_plan(500, 8000, F, 16000, 0) == (0, 500, 1000)
    # the 100 x frames limit of the default does not apply; the rate limit does
    long_root = _tree(tmp_path / "l", [("l", 8000, 100 * F + 1, 1)])
    assert WavFolderLoader(long_root, 64, 3, clip_length="window").n_clips == math.ceil((200 * F + 2) / F)
    with pytest.raises(ValueError, match="100 x"):
        WavFolderLoader(long_root, 64, 3)
    with pytest.raises(ValueError, match="100 x audio_rate"):
        WavFolderLoader(long_root, 64, 3, clip_length="window", audio_rate=79)
    with pytest.raises(ValueError, match="window_gain"):
        WavFolderLoader(long_root, 64, 3, clip_length="window", window_gain="clip")
    with pytest.raises(RuntimeError, match="no CPU path"):
        next(iter(ld))


def test_train_draws_depend_on_seed_epoch_file_and_window_only(tmp_path, monkeypatch):
    import movenet_amd.wavenet as W
    from movenet_amd.dataset import WavFolderLoader
    monkeypatch.setattr(W, "MAX_AUDIO_FRAMES", F)
    root = _tree(tmp_path, CLIPS)

    def draws(epoch, **kw):
        ld = WavFolderLoader(root, 64, kw.pop("batch_size", 3), clip_length="window", shuffle=True, **kw)
        ld.set_epoch(epoch)
        return ld, {ld.pairs[k]: ld.window_start(*ld.pairs[k]) for k in ld._order()}

    ld, e0 = draws(0)
    assert sorted(e0) == ld.pairs and len(ld) == math.ceil(11 / 3)
    for (i, w), start in e0.items():
        assert 0 <= start <= max(0, ld.n_file[i] - F)
    assert draws(0)[1] == e0                                          # reproducible for a given (seed, epoch)
    assert draws(1)[1] != e0                                          # ... another epoch, other windows
    assert len({e0[(2, w)] for w in range(4)}) > 1                    # a file's windows are separate draws
    assert draws(0, batch_size=5)[1] == e0                            # not the batch size
    both = {}
    for rank in (0, 1):                                               # not the rank: the shards' draws are e0's
        ld_r, d = draws(0, rank=rank, world_size=2)
        assert len(ld_r._order()) == 6 and all(e0[k] == v for k, v in d.items())
        both.update(d)
    assert both == e0
    # short files start at 0: max(0, n_file - frames) = 0
    assert draws(0)[0].window_start(0, 0) in range(0, 201) and WavFolderLoader(
        _tree(tmp_path / "s", [("s", 8000, 500, 1)]), 64, 3, clip_length="window").window_start(0, 0) == 0


def _as_24bit(x):
    """(frames, channels) float -> an array whose items are the 3 little-endian bytes of round(x * (2^23 - 1))"""
    v = np.round(x * 8388607.0).astype("<i4")
    raw = v.reshape(-1, 1).view(np.uint8)[:, :3].copy()
    return raw.view("V3").reshape(x.shape)


@pytest.mark.parametrize("width", [1, 2, 3])
@pytest.mark.parametrize("channels", [1, 2])
def test_read_wav_span_is_the_slice_of_the_whole_file(tmp_path, width, channels):
    from movenet_amd.dataset import read_wav_pcm16, read_wav_span, wav_file_range
    frames, rate = 5000, 22050
    x = M.signal("sines", rate, frames, channels, 3)
    stored = _as_24bit(x) if width == 3 else M.quantise(x, width)
    path = str(tmp_path / "f.wav")
    M.write_wav(path, stored, rate)
    whole, n, ch, r = read_wav_pcm16(path)
    assert (n, ch, r) == (frames, channels, rate) and whole.dtype == np.int16
    if width < 3:
        assert np.array_equal(whole.reshape(n, ch), M.as_pcm16(stored))
    else:
        v = np.round(x * 8388607.0).astype(np.int64)                   # rounded to the nearest 16-bit value
        assert np.array_equal(whole.reshape(n, ch), np.clip((v + 128) >> 8, -32768, 32767))
    for first, count in ((0, 1), (0, frames), (1234, 777), (frames - 1, 1), (4000, 1000)):
        pcm, got, c2, r2 = read_wav_span(path, first, count)
        assert (got, c2, r2) == (count, channels, rate) and pcm.dtype == np.int16
        assert np.array_equal(pcm, whole[first * ch:(first + count) * ch]), (first, count)
    assert read_wav_span(path, 4990, 100)[1] == 10                     # clipped to the file
    # the file's range: min and max of the channel mean / 32768, as the front end forms them, in bounded chunks
    import movenet_amd.dataset as D
    sums = whole.reshape(n, ch).astype(np.int64).sum(axis=1)
    want = tuple(float(np.float32(v) / (np.float32(32768.0) * np.float32(ch))) for v in (sums.min(), sums.max()))
    assert wav_file_range(path) == want
    old, D.FILE_RANGE_CHUNK = D.FILE_RANGE_CHUNK, 999
    try:
        assert wav_file_range(path) == want
    finally:
        D.FILE_RANGE_CHUNK = old


def test_window_exports_and_host_refusals():
    lib = N.lib()
    for name in ("mvn_audio_frontend_window", "mvn_audio_frontend_window_scratch_floats"):
        assert hasattr(lib, name) and name in N.SIGNATURES
    assert lib.mvn_abi_version() == 2
    assert lib.mvn_audio_frontend_window_scratch_floats(4, 2304) == 2 * 4 * 3
    assert lib.mvn_audio_frontend_window_scratch_floats(0, 2304) == 0
    Q, WIDTH = 256, 2304
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 63) // 64 * 64         # never dereferenced: the refusals come before any launch
    good = dict(pcm=p, pcm_len=10, clips=p, batch=1, classes=Q, width=WIDTH, normalize=1, y=p, scratch=p, index=p)

    def call(**over):
        a = dict(good, **over)
        return lib.mvn_audio_frontend_window(a["pcm"], a["pcm_len"], a["clips"], a["batch"], a["classes"], a["width"],
                                             a["normalize"], a["y"], a["scratch"], a["index"], None)

    for over in (dict(pcm=None), dict(clips=None), dict(y=None), dict(scratch=None), dict(index=None),
                 dict(pcm_len=0), dict(batch=0), dict(batch=65536), dict(width=0), dict(classes=1),
                 dict(classes=65537), dict(scratch=p + 4)):
        assert call(**over) == N.MVN_ERR_BAD_ARG, over
        assert "mvn_audio_frontend_window" in N.last_error(), over
    # the descriptor: 64 bytes, the fields where include/movenet_hip.h puts them
    from movenet_amd.ops import audio_clip_window_descriptors
    d = audio_clip_window_descriptors([7, 0], [100, 50], [1 << 33, 50], [2, 1], [1 << 32, 3], [10, 20],
                                      [44100, 8000], 16000, lo=[-0.5, 0.0], hi=[0.25, 0.0])
    assert d.shape == (2, 16) and d.dtype == np.int32 and d.strides == (64, 4)
    i64, f32 = d.view(np.int64), d.view(np.float32)
    assert i64[:, :4].tolist() == [[0, 7, 1 << 32, 1 << 33], [200, 0, 3, 50]]     # offsets: spans back to back
    assert d[:, 8:13].tolist() == [[100, 2, 10, 44100, 16000], [50, 1, 20, 8000, 16000]]
    assert f32[:, 13:15].tolist() == [[-0.5, 0.25], [0.0, 0.0]] and d[:, 15].tolist() == [0, 0]


def test_window_flags_parse_and_reach_the_loader(tmp_path, monkeypatch):
    import movenet_amd.wavenet as W
    from movenet_amd.config import TrainingConfig, arg_parser, config_from_args
    from movenet_amd.dataset import WavFolderLoader, get_dataloader
    assert arg_parser().parse_args([]).window_gain == "file" and TrainingConfig().window_gain == "file"
    from movenet_amd.config import ModelConfig
    from movenet_amd.pytorch_lightning_trainer import Dance2Music
    root = _tree(tmp_path, CLIPS)
    _tree(tmp_path, CLIPS[:1], "valid")
    cfg = TrainingConfig(model_config=ModelConfig(layer_size=2, stack_size=2, input_channels=64, residual_channels=32,
                                                  skip_channels=32),
                         batch_size=3, val_batch_size=3, use_video=False, model_output_path=tmp_path,
                         clip_length="window", audio_rate=16000)
    m = Dance2Music(root, cfg)
    # rows of 3000 samples (the model is built: the width enters the loaders only from here on)
    monkeypatch.setattr(W, "MAX_AUDIO_FRAMES", F)
    base = ["--dataset", root, "--use_video", "0"]
    c = config_from_args(arg_parser().parse_args(base + ["--clip_length", "window", "--window_gain", "window",
                                                         "--audio_rate", "8000"]))
    assert (c.clip_length, c.window_gain, c.audio_rate) == ("window", "window", 8000)
    back = TrainingConfig.from_json(c.to_json())
    assert (back.clip_length, back.window_gain) == ("window", "window")
    with pytest.raises(SystemExit):
        arg_parser().parse_args(base + ["--window_gain", "clip"])
    ld = get_dataloader(root, 64, 3, use_video=False, clip_length=c.clip_length, audio_rate=c.audio_rate,
                        window_gain=c.window_gain)
    assert ld.window and ld.window_gain == "window" and ld.audio_rate == 8000 and ld.file_range(0) == (0.0, 0.0)
    # through the trainer's own loader call
    tl, vl = m._loader(True), m._loader(False)
    assert tl.window and tl.train and tl.window_gain == "file" and tl.n_clips == 11
    assert vl.window and not vl.train and vl.n_clips == 2
    # per-file gain: found once per loader cache, from the file itself
    lo, hi = tl.file_range(2)
    assert lo < 0 < hi and tl.cache.ranges[2] == (lo, hi) and tl.cache is m._loader(True).cache
    assert tl.cache is not ld.cache
    with pytest.raises(ValueError, match="use_video"):
        WavFolderLoader(root, 64, 3, clip_length="window", use_video=True)
