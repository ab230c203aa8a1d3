"""GPU: the windowed by-rate front end (mvn_audio_frontend_window) through the C ABI, on buffers with sentinel bands and
an upload with poison samples around every span, and the loader that feeds it (WavFolderLoader(clip_length="window")).

Rows of 2304 columns are two full 1024-output tiles and one partial.

* A window is a crop of the whole, to the bit: against mvn_audio_frontend_var on the whole file (11 025 frames at
  44 100 Hz -> 4000 outputs: gcd(11025, 4000) = 25 gives it the 441 : 160 geometry of 44 100 -> 16 000).
* Against the float64 restatement (tests/window_reference.py), bounds taken as test_audio_frontend_gpu.py takes them:
  the kernel's waveform may deviate 4 x what a float32 numpy evaluation of the same formula deviates from float64 on
  the same windows (the margin covers sinpif / cospif against libm and another summation order -- for at most 128
  taps; a longer filter's taps the kernel sums in blocks of 128); indices within 1
  everywhere; the share of positions that differ at all at most twice float32 numpy's own.  The material is 100 windows
  tiling a file at each of 441 : 160, 2 : 3 and 1 : 1, the first and last window of a file at 100 : 1 (W = 607), and one
  window at out_first = 40 000 000 of a 120 000 000-frame file: 698 112 positions, so that float32 numpy's own share
  (1.6e-5 on the plain front end's material) is some ten positions and the factor of two is not a coin toss.  The
  given-range test holds the same windows' waveforms, quantised by the given range, to the same bounds.  The tests
  print the measured values.
"""
import math
import os

import numpy as np
import pytest
import torch

import wav_material as M
import window_reference as R
from helpers import _Guard
from movenet_amd import _native as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDTH, Q = 2304, 256
SILENCE = int((Q - 1) / 2.0 + 0.5)
REC = [("offset", "<i8"), ("span_first", "<i8"), ("out_first", "<i8"), ("file_frames", "<i8"),
       ("span_frames", "<i4"), ("channels", "<i4"), ("n_out", "<i4"), ("rate_in", "<i4"), ("rate_out", "<i4"),
       ("lo", "<f4"), ("hi", "<f4"), ("reserved", "<i4")]


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _row(pcm, rate_in, rate_out, out_first, n_out, file_frames=None, file_first=0, lo=0.0, hi=0.0):
    """One row: the window [out_first, out_first + n_out) of a file of which ``pcm`` ((frames, channels) int16) holds
    the frames from ``file_first`` on (the whole file by default); the span is the loader's own plan."""
    from movenet_amd.dataset import WavFolderLoader
    file_frames = len(pcm) if file_frames is None else file_frames
    first, span, n = WavFolderLoader.window_plan(file_frames, rate_in, n_out, rate_out, out_first)
    assert n == n_out and first >= file_first
    return dict(span=pcm[first - file_first:first - file_first + span], span_first=first, span_frames=span,
                file_frames=file_frames, channels=pcm.shape[1], out_first=out_first, n_out=n_out, rate_in=rate_in,
                rate_out=rate_out, lo=lo, hi=hi)


def _descriptors(rows, gap):
    """(B, 16) int32 descriptors with every span behind ``gap`` samples of poison, and the spans' offsets"""
    from movenet_amd.ops import audio_clip_window_descriptors
    offsets, at = [], gap
    for r in rows:
        offsets.append(at)
        at += r["span"].size + gap
    f = lambda k: [r[k] for r in rows]
    return audio_clip_window_descriptors(f("span_first"), f("span_frames"), f("file_frames"), f("channels"),
                                         f("out_first"), f("n_out"), f("rate_in"), f("rate_out"), lo=f("lo"),
                                         hi=f("hi"), offsets=offsets), offsets, at


def _window(rows, normalize=False, width=WIDTH, poison=12345, gap=777, desc=None):
    """mvn_audio_frontend_window on guarded buffers.  The upload: ``gap`` poison samples, then every span followed by
    ``gap`` more, so that each span lies at a non-zero offset between poison.  ``desc`` replaces the descriptors
    (same upload).  Returns (idx, y)."""
    lib = N.lib()
    made, offsets, total = _descriptors(rows, gap)
    desc = made if desc is None else desc
    pcm = np.full(total, poison, dtype=np.int16)
    for r, o in zip(rows, offsets):
        assert o > 0 and r["span"].shape == (r["span_frames"], r["channels"])
        pcm[o:o + r["span"].size] = r["span"].reshape(-1)
    B = len(rows)
    guard = _Guard(front=True)
    d_pcm = torch.from_numpy(pcm).to(DEV)
    y = guard.new((B, width), fill=-7.0, name="y")
    idx = guard.new((B, width), fill=-77, name="index", dtype=torch.int32)
    scratch = guard.new((max(lib.mvn_audio_frontend_window_scratch_floats(B, width), 2),), fill=float("nan"),
                        name="scratch")
    d = torch.from_numpy(np.ascontiguousarray(desc)).to(DEV)
    rc = lib.mvn_audio_frontend_window(d_pcm.data_ptr(), d_pcm.numel(), d.data_ptr(), B, Q, width, int(normalize),
                                       y.data_ptr(), scratch.data_ptr(), idx.data_ptr(), _stream())
    assert rc == N.MVN_OK, N.last_error()
    guard.check("mvn_audio_frontend_window")
    return idx, y


def _bits(t):
    return t.contiguous().view(torch.int32)


def _pcm(kind, rate, frames, channels, seed):
    return M.as_pcm16(M.quantise(M.signal(kind, rate, frames, channels, seed), 2))


# ---- 1. a window is a crop, to the bit ---------------------------------------------------------------------------------

CROPS = ((0, 2304), (1000, 3304), (1696, 4000), (3999, 4000), (0, 4000))


def test_a_window_is_a_crop_of_the_whole_file_to_the_bit():
    from movenet_amd.ops import audio_clip_var_descriptors, audio_frontend_var
    rate_in, rate_out, frames, n_file, width = 44100, 16000, 11025, 4000, 4096
    pcm = _pcm("sines", rate_in, frames, 2, 4)
    assert R.n_file(frames, rate_in, rate_out) == n_file and math.gcd(frames, n_file) == 25
    assert (frames // 25, n_file // 25) == R.geometry(rate_in, rate_out)[:2] == (441, 160)
    d_pcm = torch.from_numpy(pcm.reshape(-1)).to(DEV)
    d_desc = torch.from_numpy(audio_clip_var_descriptors([frames], [2], [n_file])).to(DEV)
    whole = {nz: audio_frontend_var(d_pcm, d_desc, Q, width, normalize=nz, return_waveform=True) for nz in (False, True)}
    rows = [_row(pcm, rate_in, rate_out, a, b - a) for a, b in CROPS]
    # only the planned span goes up: the windows inside the file need a part of it
    assert [r["span_frames"] < frames for r in rows] == [True, True, True, True, False]
    assert rows[3]["span_frames"] == frames - (3999 * 441 // 160 - R.geometry(rate_in, rate_out)[3]) == 20
    idx, y = _window(rows, normalize=False, width=width)
    want_i, want_y = whole[False]
    for b, (a, e) in enumerate(CROPS):
        n = e - a
        assert torch.equal(_bits(y[b, :n]), _bits(want_y[0, a:e])), (a, e)
        assert torch.equal(idx[b, :n], want_i[0, a:e]), (a, e)
        assert bool((idx[b, n:] == SILENCE).all()) and bool((_bits(y[b, n:]) == 0).all()), (a, e)
    # normalised: the full window is the whole file's row
    idx1, y1 = _window(rows[4:], normalize=True, width=width)
    assert torch.equal(idx1[0], whole[True][0][0]) and torch.equal(_bits(y1[0]), _bits(whole[True][1][0]))
    assert not torch.equal(idx1[0], idx[4])


def test_windows_of_a_long_filter_are_crops_of_the_whole_file_by_the_same_call(float64_material, float64_results):
    """100 : 1, 1216 taps: the taps are summed in blocks, so the bits are not mvn_audio_frontend_var's; a window is
    still a crop, to the bit, of this call's own row over the whole file"""
    rows = float64_material["100:1"][0]
    file = rows[0]["file_frames"]
    span = np.zeros((file, 1), dtype=np.int16)
    for r in rows:                                                    # the two spans together are the whole file
        span[r["span_first"]:r["span_first"] + r["span_frames"]] = r["span"]
    assert rows[0]["span_first"] + rows[0]["span_frames"] > rows[1]["span_first"]
    whole = dict(rows[0], span=span, span_first=0, span_frames=file, out_first=0, n_out=4000)
    idx, y = _window([whole], normalize=False, width=4096)
    for r, (_, got_y) in zip(rows, [_window([r], normalize=False) for r in rows]):
        a = r["out_first"]
        assert torch.equal(_bits(got_y[0]), _bits(y[0, a:a + WIDTH])), a
    assert bool((_bits(y[0, 4000:]) == 0).all()) and bool((idx[0, 4000:] == SILENCE).all())


# ---- 2. against float64 --------------------------------------------------------------------------------------------------

def _quantise_range(y, lo, hi, dtype):
    """wav_material.quantise_np with the (min, max) given"""
    y = y.astype(dtype)
    y = (y - dtype(lo)) / (dtype(hi) - dtype(lo))
    y = y * dtype(2.0) - dtype(1.0)
    mu = dtype(Q - 1)
    z = np.sign(y) * np.log1p(mu * np.abs(y)) / np.log1p(mu)
    return np.clip(((z + dtype(1.0)) / dtype(2.0) * mu + dtype(0.5)).astype(np.int64), 0, Q - 1)


def _references(row):
    """y and indices (normalised by the window's own range) of a row in float64 and float32 numpy"""
    out = {}
    for name, dt in (("64", np.float64), ("32", np.float32)):
        m = M.downmix_np(row["span"], dt)
        y = R.resample_window_np(m, row["span_first"], row["file_frames"], row["rate_in"], row["rate_out"],
                                 row["out_first"], row["n_out"], dtype=dt)
        out["y" + name] = y
        out["q" + name] = M.quantise_np(y, Q, True, dt)
    return out


def _requantised(ref, lo, hi):
    """the same waveforms, their indices by the given range"""
    return dict(ref, q64=_quantise_range(ref["y64"], lo, hi, np.float64),
                q32=_quantise_range(ref["y32"], lo, hi, np.float32))


def _tiling(rate_in, rate_out, channels, seed, windows=100):
    """the windows that tile a file of ``windows`` x WIDTH outputs, the first and the last with taps outside the file"""
    orig, new, _, _ = R.geometry(rate_in, rate_out)
    frames = windows * WIDTH * orig // new
    assert R.n_file(frames, rate_in, rate_out) == windows * WIDTH
    pcm = _pcm("sines", rate_in, frames, channels, seed)
    return [_row(pcm, rate_in, rate_out, w * WIDTH, WIDTH) for w in range(windows)]


@pytest.fixture(scope="module")
def float64_material():
    groups = {"441:160": _tiling(44100, 16000, 2, 1), "2:3": _tiling(8000, 12000, 1, 2),
              "1:1": _tiling(16000, 16000, 2, 3)}
    rate = 1_600_000                                                  # 100 : 1, W = 607
    assert R.geometry(rate, 16000)[:2] == (100, 1) and R.geometry(rate, 16000)[3] == 607
    pcm = _pcm("sines", rate, 400_000, 1, 4)
    groups["100:1"] = [_row(pcm, rate, 16000, 0, WIDTH), _row(pcm, rate, 16000, 4000 - WIDTH, WIDTH)]
    # far into a long file: only the span is real data
    out_first, file_frames = 40_000_000, 120_000_000
    first, last = R.tap_range(file_frames, 44100, 16000, out_first, WIDTH)
    far = _pcm("sines", 44100, last - first + 1, 2, 5)
    groups["far"] = [_row(far, 44100, 16000, out_first, WIDTH, file_frames=file_frames, file_first=first)]
    assert out_first * 441 > 1 << 32
    return {k: (rows, [_references(r) for r in rows]) for k, rows in groups.items()}


def _fp32_numpy(groups):
    """(waveform tolerance, cap on the differing share, positions) from float32 numpy's own distance to float64 on
    ``groups``, after the conditions the caps rest on (the CPU half)"""
    refs = [r for _, rs in groups.values() for r in rs]
    total = sum(len(r["y64"]) for r in refs)
    fp32_dev = max(float(np.abs(r["y32"].astype(np.float64) - r["y64"]).max()) for r in refs)
    fp32_differ = sum(int((r["q32"] != r["q64"]).sum()) for r in refs)
    print(f"fp32 numpy: deviation {fp32_dev:.3e}, {fp32_differ} of {total} positions differ ({fp32_differ / total:.3e})")
    assert 0 < fp32_dev < 1e-6 and fp32_differ / total < 1e-4
    return 4.0 * fp32_dev, 2.0 * fp32_differ / total, total


def _index_distance(rows, refs, idx):
    idx = idx.cpu().numpy()
    return np.concatenate([np.abs(idx[b, :r["n_out"]].astype(np.int64) - ref["q64"])
                           for b, (r, ref) in enumerate(zip(rows, refs))])


def _hold_indices(groups, got):
    """indices within 1 everywhere, the differing share at most twice float32 numpy's own, over all of ``groups``"""
    _, cap, total = _fp32_numpy(groups)
    differ = 0
    for name, (rows, refs) in groups.items():
        dq = _index_distance(rows, refs, got[name][0])
        differ += int((dq != 0).sum())
        print(f"{name}: {len(rows)} windows, indices differ at {int((dq != 0).sum())} positions, by {int(dq.max())} "
              "at most")
        assert dq.max() <= 1, name
    print(f"kernel: {differ} of {total} positions differ ({differ / total:.3e}, cap {cap:.3e})")
    assert differ / total <= cap


@pytest.fixture(scope="module")
def float64_results(float64_material):
    return {name: _window(rows, normalize=True) for name, (rows, _) in float64_material.items()}


@pytest.mark.parametrize("name", ["441:160", "2:3", "1:1", "100:1", "far"])
def test_window_waveforms_match_the_float64_restatement(float64_material, float64_results, name):
    """At 100 : 1 a sample is the sum of 2 W + 2 = 1216 taps; the kernel sums them in blocks of 128.  One
    chain of fmaf over all of them deviated 1.420e-06 there on an MI355X and missed the tolerance (9.251e-07 = 4 x
    float32 numpy's 2.313e-07); the blocked sum measures 3.621e-07 (441:160 2.844e-07, 2:3 2.076e-07, 1:1 1.809e-07,
    far 2.112e-07)."""
    tol, _, _ = _fp32_numpy(float64_material)
    rows, refs = float64_material[name]
    y = float64_results[name][1].cpu().numpy()
    dev = max(float(np.abs(y[b, :r["n_out"]].astype(np.float64) - ref["y64"]).max())
              for b, (r, ref) in enumerate(zip(rows, refs)))
    print(f"{name}: {len(rows)} windows, waveform deviation {dev:.3e} (tolerance {tol:.3e})")
    assert dev <= tol, (name, dev, tol)


def test_window_indices_match_the_float64_restatement(float64_material, float64_results):
    _hold_indices(float64_material, float64_results)
    rows = float64_material["441:160"][0]
    assert rows[0]["span_first"] == 0 and rows[-1]["span_first"] + rows[-1]["span_frames"] == rows[-1]["file_frames"]


# ---- 3. a given range ------------------------------------------------------------------------------------------------------

def test_given_range_normalises_and_a_range_not_given_falls_back(float64_material):
    lo, hi = float(np.float32(-0.9)), float(np.float32(0.7))
    groups = {name: ([dict(r, lo=lo, hi=hi) for r in rows], [_requantised(ref, lo, hi) for ref in refs])
              for name, (rows, refs) in float64_material.items()}
    got = {name: _window(rows, normalize=True) for name, (rows, _) in groups.items()}
    _hold_indices(groups, got)
    # the range changes the indices and leaves the waveform alone; normalize = 0 ignores it
    base_rows = float64_material["441:160"][0][:3]
    own_i, own_y = _window(base_rows, normalize=True)
    assert not torch.equal(got["441:160"][0][:3], own_i) and torch.equal(_bits(got["441:160"][1][:3]), _bits(own_y))
    raw_i, _ = _window(base_rows, normalize=False)
    assert torch.equal(_window([dict(r, lo=lo, hi=hi) for r in base_rows], normalize=False)[0], raw_i)
    # hi <= lo, or no range at all (NaN, infinite): the window's own
    for l, h in ((0.3, -0.3), (0.25, 0.25), (float("nan"), 1.0), (-float("inf"), 1.0), (-3e38, 3e38)):
        idx, _ = _window([dict(r, lo=l, hi=h) for r in base_rows], normalize=True)
        assert torch.equal(idx, own_i), (l, h)
    # a silent window stays at the silence class: its own range is empty, and a range around zero maps 0 to 0
    silent = np.zeros((11025, 2), dtype=np.int16)
    rows = [_row(silent, 44100, 16000, 1000, WIDTH), _row(silent, 44100, 16000, 1000, WIDTH, lo=-0.5, hi=0.5),
            _row(silent, 44100, 16000, 3000, 1000)]
    idx, y = _window(rows, normalize=True)
    assert bool((idx == SILENCE).all()) and bool((_bits(y) == 0).all())


# ---- 4. refusals on the device -----------------------------------------------------------------------------------------

def _refusal_rows():
    pcm = _pcm("sines", 44100, 30000, 2, 6)                           # n_file = 10885
    mono = _pcm("chirp", 8000, 4000, 1, 7)
    return [_row(pcm, 44100, 16000, 3000, WIDTH), _row(pcm, 44100, 16000, 5000, 1500, lo=-0.8, hi=0.8),
            _row(mono, 8000, 12000, 6000 - 1025, 1025)]


REFUSALS = (
    ("span past the upload", dict(offset="past")),
    ("negative offset", dict(offset=-1)),
    ("no span", dict(span_frames=0)),
    ("n_out = 0", dict(n_out=0)),
    ("n_out = width + 1", dict(n_out=WIDTH + 1)),
    ("rate_in = 0", dict(rate_in=0)),
    ("rate_out < 0", dict(rate_out=-16000)),
    ("channels = 0", dict(channels=0)),
    ("a ratio of 200 : 1", dict(rate_in=3_200_000)),
    ("out_first < 0", dict(out_first=-1)),
    ("window past the file's end", dict(out_first=10885 - 1500 + 1)),
    ("no file", dict(file_frames=0)),
    ("span starts one frame late", dict(span_first="+1")),
    ("span ends one frame early", dict(span_frames="-1")),
)


@pytest.fixture(scope="module")
def refusal_base():
    rows = _refusal_rows()
    return rows, _window(rows, normalize=True), _window([rows[0], rows[2]], normalize=True)


@pytest.mark.parametrize("what,change", REFUSALS, ids=[w for w, _ in REFUSALS])
def test_refused_rows_are_marked_and_the_others_keep_their_bits(refusal_base, what, change):
    rows, (good_i, good_y), (pair_i, pair_y) = refusal_base
    # the rows of the full batch are those of a batch without the middle row
    assert torch.equal(good_i[0], pair_i[0]) and torch.equal(good_i[2], pair_i[1])
    assert torch.equal(_bits(good_y[0]), _bits(pair_y[0])) and torch.equal(_bits(good_y[2]), _bits(pair_y[1]))
    desc, _, total = _descriptors(rows, 777)
    rec = desc.view(REC).reshape(len(rows))
    for field, value in change.items():
        if value == "past":
            value = total - 10
        elif value == "+1":
            value = int(rec[field][1]) + 1
        elif value == "-1":
            value = int(rec[field][1]) - 1
        rec[field][1] = value
    out = []
    for poison in (12345, -321):      # the poison around the spans (and all of the refused row's) is never read
        idx, y = _window(rows, normalize=True, desc=desc, poison=poison)
        assert bool((idx[1] == -1).all()) and bool((_bits(y[1]) == 0).all()), what
        for b in (0, 2):
            assert torch.equal(idx[b], good_i[b]) and torch.equal(_bits(y[b]), _bits(good_y[b])), (what, b)
        out.append((idx, y))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(_bits(out[0][1]), _bits(out[1][1]))


def test_every_refusal_rule_is_among_the_cases():
    fields = {f for _, c in REFUSALS for f in c}
    assert {"offset", "n_out", "rate_in", "rate_out", "channels", "out_first", "span_first", "span_frames"} <= fields
    assert R.geometry(3_200_000, 16000)[3] == 1213                    # the ratio whose 64-output window is too long


# ---- 5. determinism --------------------------------------------------------------------------------------------------------

def test_two_calls_give_the_same_bits_and_rows_do_not_depend_on_their_place():
    rows = _refusal_rows()
    a_i, a_y = _window(rows, normalize=True)
    b_i, b_y = _window(rows, normalize=True)
    assert torch.equal(a_i, b_i) and torch.equal(_bits(a_y), _bits(b_y))
    order = [2, 0, 1]
    p_i, p_y = _window([rows[k] for k in order], normalize=True, gap=1031)
    for at, k in enumerate(order):
        assert torch.equal(p_i[at], a_i[k]) and torch.equal(_bits(p_y[at]), _bits(a_y[k])), k
    one_i, one_y = _window(rows[1:2], normalize=True)
    assert torch.equal(one_i[0], a_i[1]) and torch.equal(_bits(one_y[0]), _bits(a_y[1]))


# ---- 6. the loader end to end ------------------------------------------------------------------------------------------

FILES = (("long_44k", 44100, 30000, 2), ("short_8k", 8000, 500, 1), ("two_16k", 16000, 4000, 1))   # 10885, 1000, 4000
N_FILE, WINDOWS = (10885, 1000, 4000), (5, 1, 2)


def _wav_tree(root):
    for split in ("train", "valid"):
        d = os.path.join(str(root), split, "a")
        os.makedirs(d)
        for seed, (name, rate, frames, ch) in enumerate(FILES):
            M.write_wav(os.path.join(d, name + ".wav"), M.quantise(M.signal("sines", rate, frames, ch, seed), 2), rate)
    return str(root)


def _whole_file_indices(path, q):
    """the file's full by-rate indices from ONE call, normalised by the file's own range"""
    from movenet_amd.dataset import read_wav_pcm16, resampled_frames, wav_file_range
    from movenet_amd.ops import audio_clip_window_descriptors, audio_frontend_window
    pcm, frames, ch, rate = read_wav_pcm16(path)
    n = resampled_frames(frames, rate, 16000)
    lo, hi = wav_file_range(path)
    desc = audio_clip_window_descriptors([0], [frames], [frames], [ch], [0], [n], [rate], 16000, lo=[lo], hi=[hi])
    return audio_frontend_window(torch.from_numpy(pcm).to(DEV), torch.from_numpy(desc).to(DEV), q, n)[0]


def test_loader_windows_end_to_end(tmp_path, monkeypatch):
    import movenet_amd.wavenet as W
    from movenet_amd.dataset import WavFolderLoader, get_dataloader, read_wav_span
    from movenet_amd.ops import audio_clip_window_descriptors, audio_frontend_window
    monkeypatch.setattr(W, "MAX_AUDIO_FRAMES", WIDTH)
    root = _wav_tree(tmp_path / "wavs")
    q = 64
    silence = int((q - 1) / 2.0 + 0.5)
    whole = [_whole_file_indices(os.path.join(root, "valid", "a", name + ".wav"), q) for name, _, _, _ in FILES]
    assert [len(w) for w in whole] == list(N_FILE)
    # validation windows, concatenated, are the file's full by-rate indices
    vl = get_dataloader(root, q, batch_size=3, train=False, use_video=False, device=DEV, clip_length="window")
    assert [vl.window_count(h["frames"], h["rate"], WIDTH, 16000) for _, _, h in vl.index] == list(WINDOWS)
    for epoch in range(2):
        parts, starts = {i: [] for i in range(len(FILES))}, {i: [] for i in range(len(FILES))}
        rows = 0
        for batch in vl:
            B = batch.audio.shape[0]
            assert tuple(batch.audio.shape) == (B, q, WIDTH) and bool((batch.audio.sum(1) == 1).all())
            idx = batch.audio.argmax(1)
            for b in range(B):
                i = vl.filepaths.index(batch.filepaths[b])
                n = batch.lengths[b]
                assert 1 <= n <= WIDTH and bool((idx[b, n:] == silence).all())
                assert batch.info[b]["audio_fps"] == float(FILES[i][1])
                parts[i].append(idx[b, :n])
                starts[i].append(batch.info[b]["out_first"])
            rows += B
        assert rows == sum(WINDOWS) and len(vl) == math.ceil(rows / 3)
        for i in range(len(FILES)):
            assert starts[i] == [w * WIDTH for w in range(WINDOWS[i])]
            assert torch.equal(torch.cat(parts[i]), whole[i].to(torch.int64)), (epoch, i)
        stats = vl.cache_stats()
        assert (stats["hits"], stats["misses"], stats["clips"]) == (epoch * rows, rows, rows)
    # a train epoch: sum of n_i rows, each the file's own samples at its draw, lengths as under native
    tl = get_dataloader(root, q, batch_size=4, train=True, use_video=False, device=DEV, clip_length="window",
                        shuffle=True)
    seen = {}
    for epoch in range(2):
        tl.set_epoch(epoch)
        rows = 0
        for batch in tl:
            idx = batch.audio.argmax(1)
            for b in range(idx.shape[0]):
                i = tl.filepaths.index(batch.filepaths[b])
                o, n = batch.info[b]["out_first"], batch.lengths[b]
                assert 0 <= o <= max(0, N_FILE[i] - WIDTH) and n == min(WIDTH, N_FILE[i] - o)
                assert torch.equal(idx[b, :n], whole[i][o:o + n].to(torch.int64)), (epoch, i, o)
                assert bool((idx[b, n:] == silence).all())
                seen.setdefault(epoch, []).append((i, o))
            rows += idx.shape[0]
        assert rows == sum(WINDOWS) == tl.n_clips
    assert sorted(seen[0]) != sorted(seen[1]) and tl.cache_stats()["clips"] == 0      # train windows pass the cache by
    # window_gain="window": each window by its own range, so the rows differ from the file-gain ones
    wl = WavFolderLoader(root, q, 3, train=False, device=DEV, clip_length="window", window_gain="window")
    first = next(iter(wl))
    assert first.lengths == [WIDTH] * 3 and first.info[1]["out_first"] == WIDTH
    path = os.path.join(root, "valid", "a", FILES[0][0] + ".wav")
    span_first, span, n = WavFolderLoader.window_plan(FILES[0][2], FILES[0][1], WIDTH, 16000, WIDTH)
    pcm = read_wav_span(path, span_first, span)[0]
    desc = audio_clip_window_descriptors([span_first], [span], [FILES[0][2]], [2], [WIDTH], [n], [FILES[0][1]], 16000)
    own = audio_frontend_window(torch.from_numpy(pcm).to(DEV), torch.from_numpy(desc).to(DEV), q, WIDTH)
    assert torch.equal(first.audio.argmax(1)[1], own[0].to(torch.int64))
    assert not torch.equal(own[0], whole[0][WIDTH:2 * WIDTH])
    # batch_subsample_frac crops rows and lengths as under native
    cl = WavFolderLoader(root, q, 8, train=False, device=DEV, clip_length="window", batch_subsample_frac=0.25)
    batch = next(iter(cl))
    n = math.ceil(WIDTH * 0.25)
    assert tuple(batch.audio.shape) == (8, q, n)
    full = [WIDTH] * 4 + [N_FILE[0] - 4 * WIDTH, N_FILE[1], WIDTH, N_FILE[2] - WIDTH]
    start = [s for s in range(WIDTH - n + 1) if WavFolderLoader.cropped_lengths(full, s, n) == batch.lengths]
    assert start and any(torch.equal(batch.audio.argmax(1)[0], whole[0][s:s + n].to(torch.int64)) for s in start)


def test_trainer_fit_on_windows_with_mel(tmp_path, monkeypatch):
    """two optimizer steps of Trainer.fit with --use_mel 1 --clip_length window: the lengths reach the steps, which log
    a finite loss and the share of loss columns that count"""
    import movenet_amd.wavenet as W
    from movenet_amd.config import ModelConfig, TrainingConfig, arg_parser, config_from_args
    from movenet_amd.pytorch_lightning_trainer import Dance2Music, Trainer
    root = _wav_tree(tmp_path / "wavs")
    args = arg_parser().parse_args(["--dataset", root, "--use_video", "0", "--clip_length", "window", "--use_mel", "1"])
    c = config_from_args(args)
    assert (c.clip_length, c.window_gain, c.use_mel) == ("window", "file", True)
    cfg = TrainingConfig(model_config=ModelConfig(layer_size=2, stack_size=2, input_channels=64, residual_channels=32,
                                                  skip_channels=32),
                         batch_size=8, val_batch_size=8, n_epochs=2, use_video=False, optimizer="AdamW",
                         learning_rate=1e-3, weight_decay=0.0, scheduler=None, model_output_path=tmp_path,
                         loss_rule="model", clip_length="window", audio_rate=16000, use_mel=True, mel_bins=8,
                         mel_fft=64, mel_hop=16)
    m = Dance2Music(root, cfg)
    # rows of 2304 samples instead of 160 000 (the model is built: the width enters the loaders only from here on)
    monkeypatch.setattr(W, "MAX_AUDIO_FRAMES", WIDTH)
    tr = Trainer(max_epochs=2, default_root_dir=None, gradient_clip_val=0.0, limit_val_batches=1)
    tr.fit(m)
    assert len(tr.history) == 2                                        # 8 (file, window) rows: one batch an epoch
    rf = m.model.receptive_fields
    for h in tr.history:
        assert math.isfinite(h["train_loss"]) and 0.0 < h["train_valid_frac"] < 1.0
    # the validation rows tile the files: every real sample behind a row's first rf counts
    lengths = [WIDTH] * 4 + [N_FILE[0] - 4 * WIDTH, N_FILE[1], WIDTH, N_FILE[2] - WIDTH]
    want = sum(max(n - rf, 0) for n in lengths) / (8 * (WIDTH - rf))
    assert abs(m.logged["val_valid_frac"] - want) < 1e-9 and math.isfinite(float(m.logged["val_loss"]))
