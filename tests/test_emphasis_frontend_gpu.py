"""GPU: pre-emphasis in the audio front end (mvn_audio_frontend_emph, ``preemphasis=a`` of the three ops) against the
float64 restatement of tests/emphasis_reference.py.

The reference row is built from what the UN-emphasised call returns -- its fp32 resample y and that row's (min, max), or
the given range -- so what is pinned is the new kernel's own arithmetic: the two normalisations, the product, the
difference and the quotient.  The bound on e is 1e-6, derived: at most six float32 roundings on magnitudes <= 2, each
<= 2^-24 * 2 = 1.2e-7.  The class indices are then EXACTLY the clamped mu-law of the e the kernel wrote."""
import numpy as np
import pytest
import torch

import emphasis_reference as R
from movenet_amd import ops
from movenet_amd.dataset import WavFolderLoader

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Q = 256
SILENCE = 128          # (int)((Q - 1) / 2.0f + 0.5f)
BOUND = 1e-6
COEFS = [0.97, 0.5]
WIDTH = 2100
N_OUT = [1, 1024, 1025, 2100]   # no predecessor; exactly one tile; the predecessor in the previous tile; two boundaries


def _pcm(frames, channels, seed):
    """(frames * channels,) int16: a few sines under noise, loud enough to use the range"""
    rng = np.random.default_rng(seed)
    t = np.arange(frames)[:, None]
    x = 0.5 * np.sin(2 * np.pi * (0.013 + 0.004 * np.arange(channels)) * t) + 0.2 * rng.standard_normal((frames, channels))
    return np.round(np.clip(x, -1, 1) * 30000).astype(np.int16).reshape(-1)


def _normalised(y, normalize, lo=None, hi=None):
    """vn of one row's N resampled values in float64: min-max by the fp32 range (the row's own unless given)"""
    y = np.asarray(y, dtype=np.float64)
    if not normalize:
        return y
    mn, mx = (np.float64(y.min()), np.float64(y.max())) if lo is None else (np.float64(lo), np.float64(hi))
    if mx == mn:
        return y
    return (y - mn) / (mx - mn) * 2.0 - 1.0


def _check_rows(e, idx, y, lengths, a, normalize, ranges=None):
    """(a) e against the reference row by row, 0 behind a row's N; (b) idx == clamp(mu_law_encode(e)), silence behind N"""
    e_host, idx_host, y_host = e.cpu().numpy(), idx.cpu().numpy(), y.cpu().numpy()
    enc = ops.mu_law_encode(e, Q).clamp(0, Q - 1).cpu().numpy()
    worst = 0.0
    for b, n in enumerate(lengths):
        lo, hi = (None, None) if ranges is None else ranges[b]
        want = R.preemphasise(_normalised(y_host[b, :n], normalize, lo, hi), a)
        worst = max(worst, float(np.abs(e_host[b, :n] - want).max()))
        assert np.all(e_host[b, n:] == 0.0)
        assert np.array_equal(idx_host[b, :n], enc[b, :n]), (b, np.flatnonzero(idx_host[b, :n] != enc[b, :n])[:5])
        assert np.all(idx_host[b, n:] == SILENCE)
    print(f"a={a} normalize={normalize}: max |e - e_ref| = {worst:.3e} (bound {BOUND:g})")
    assert worst <= BOUND, worst


@pytest.fixture(scope="module")
def var_batch():
    """pcm and descriptors of the by-rate batch: four rows of N_OUT columns and a fifth the kernel refuses"""
    frames = [3] + [int(1.37 * n) + 5 for n in N_OUT[1:]] + [10]
    channels = [1, 2, 1, 2, 1]
    pcm = torch.from_numpy(np.concatenate([_pcm(f, c, 10 + i) for i, (f, c) in enumerate(zip(frames, channels))]))
    desc = ops.audio_clip_var_descriptors(frames, channels, N_OUT + [WIDTH + 1])
    return pcm.to(DEV), torch.from_numpy(desc).to(DEV)


@pytest.mark.parametrize("normalize", [True, False], ids=["normalised", "raw"])
@pytest.mark.parametrize("a", COEFS)
def test_by_rate_rows_across_tile_boundaries(var_batch, a, normalize):
    pcm, desc = var_batch
    idx0, y0 = ops.audio_frontend_var(pcm, desc, Q, WIDTH, normalize=normalize, return_waveform=True)
    idx, y, e = ops.audio_frontend_var(pcm, desc, Q, WIDTH, normalize=normalize, return_waveform=True, preemphasis=a)
    assert torch.equal(y, y0)                                     # the resample launch is the one it was
    assert bool((idx[4] == -1).all()) and bool((idx0[4] == -1).all()) and bool((e[4] == 0).all())
    _check_rows(e[:4], idx[:4], y[:4], N_OUT, a, normalize)
    assert not torch.equal(idx[1:4], idx0[1:4])                   # emphasis does something
    # (c) coefficient 0 is today's call, to the bit -- and without return_waveform the indices alone come back
    again = ops.audio_frontend_var(pcm, desc, Q, WIDTH, normalize=normalize, preemphasis=0.0)
    assert torch.equal(again, idx0)
    assert torch.equal(ops.audio_frontend_var(pcm, desc, Q, WIDTH, normalize=normalize, preemphasis=a), idx)


@pytest.mark.parametrize("a", COEFS)
def test_fixed_length_form(a):
    n_out, frames, channels = 1025, [1400, 3000], [2, 1]
    pcm = torch.from_numpy(np.concatenate([_pcm(f, c, 20 + i) for i, (f, c) in enumerate(zip(frames, channels))])).to(DEV)
    idx0, y0 = ops.audio_frontend(pcm, frames, channels, Q, n_out=n_out, return_waveform=True)
    idx, y, e = ops.audio_frontend(pcm, frames, channels, Q, n_out=n_out, return_waveform=True, preemphasis=a)
    assert torch.equal(y, y0) and tuple(e.shape) == (2, n_out)
    _check_rows(e, idx, y, [n_out, n_out], a, True)
    assert torch.equal(ops.audio_frontend(pcm, frames, channels, Q, n_out=n_out, preemphasis=0.0), idx0)


@pytest.mark.parametrize("a", COEFS)
def test_window_in_mid_file_with_a_given_range(a):
    """one window that starts in the middle of its file, normalised by a file range lo < hi, and one by its own range;
    the window's first column has no predecessor: vn[-1] = 0, whatever the file held in front of it"""
    rate_in, rate_out, file_frames, width = 22050, 16000, 40000, 1500
    full = _pcm(file_frames, 2, 31).reshape(file_frames, 2)
    rows = [(5000, np.float32(-0.5), np.float32(0.7)), (11111, np.float32(0.0), np.float32(0.0))]
    plans = [WavFolderLoader.window_plan(file_frames, rate_in, width, rate_out, first) for first, _, _ in rows]
    assert all(p[0] > 0 and p[2] == width for p in plans)   # mid-file: the span starts inside the file
    spans = [full[p[0]:p[0] + p[1]].reshape(-1) for p in plans]
    desc = ops.audio_clip_window_descriptors([p[0] for p in plans], [p[1] for p in plans], [file_frames] * 2, [2, 2],
                                             [r[0] for r in rows], [p[2] for p in plans], [rate_in] * 2, rate_out,
                                             lo=[r[1] for r in rows], hi=[r[2] for r in rows])
    pcm, d = torch.from_numpy(np.concatenate(spans)).to(DEV), torch.from_numpy(desc).to(DEV)
    idx0, y0 = ops.audio_frontend_window(pcm, d, Q, width, return_waveform=True)
    idx, y, e = ops.audio_frontend_window(pcm, d, Q, width, return_waveform=True, preemphasis=a)
    assert torch.equal(y, y0)
    _check_rows(e, idx, y, [width, width], a, True, ranges=[(rows[0][1], rows[0][2]), (None, None)])
    assert torch.equal(ops.audio_frontend_window(pcm, d, Q, width, preemphasis=0.0), idx0)


def test_loader_passes_the_coefficient_to_its_front_end(tmp_path):
    """WavFolderLoader(preemphasis=a): the batch's classes are the emphasised ones, from a cache of their own"""
    import wave
    folder = tmp_path / "train" / "tones"
    folder.mkdir(parents=True)
    for i in range(2):
        with wave.open(str(folder / f"c{i}.wav"), "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(_pcm(20000, 1, 40 + i).tobytes())
    plain = WavFolderLoader(tmp_path, Q, batch_size=2, device=DEV)
    emph = WavFolderLoader(tmp_path, Q, batch_size=2, device=DEV, preemphasis=0.97)
    assert plain.cache is not emph.cache and emph.preemphasis == 0.97
    a, b = next(iter(plain)).audio.argmax(1), next(iter(emph)).audio.argmax(1)
    assert a.shape == b.shape and not torch.equal(a, b)
    clips = [_pcm(20000, 1, 40 + i) for i in range(2)]
    want = ops.audio_frontend(torch.from_numpy(np.concatenate(clips)).to(DEV), [20000, 20000], [1, 1], Q,
                              n_out=plain.frames, preemphasis=0.97)
    assert torch.equal(b.to(torch.int32), want)
    with pytest.raises(ValueError, match="preemphasis"):
        WavFolderLoader(tmp_path, Q, batch_size=2, device=DEV, preemphasis=1.0)
