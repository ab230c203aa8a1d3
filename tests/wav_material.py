"""Test material and the numpy restatement for the WAV-folder source (a helper, not a test).

* ``write_tree`` writes small WAV trees (``<root>/train/<context>/*.wav``, ``<root>/valid/...``) from closed-form
  signals -- sums of a few sines, a chirp, a silent clip -- with the standard library's ``wave``: mono and stereo,
  8- and 16-bit, 8 000 / 22 050 / 44 100 / 48 000 Hz, one length coprime to 160 000.  Nothing is committed as a
  binary fixture: the files are made at test time.
* ``frontend_np`` restates the loader's arithmetic (channel mean, sinc_interp_hann resample of the whole clip to N
  frames with lowpass_filter_width 6 and roll-off 0.99, min-max normalisation, mu-law) in numpy, in float64 (the
  definition the kernel is held to) or in float32 (the same formula at the kernel's precision: what the kernel's
  tolerance is derived from).
* ``interpolation_error_bound`` derives, from the window alone, how far a resampled sine may lie from the same sine
  at the new rate.
"""
from __future__ import annotations

import math
import os
import wave

import numpy as np

MATERIAL = (
    # name, context, rate, frames, channels, sample width (bytes), kind
    ("sines_8k_mono", "speech", 8000, 8000, 1, 2, "sines"),
    ("sines_22k_stereo", "speech", 22050, 33075, 2, 2, "sines"),
    ("sines_44k_stereo", "music", 44100, 88200, 2, 2, "sines"),
    ("coprime_44k_stereo", "music", 44100, 200001, 2, 2, "sines"),   # gcd(200001, 160000) = 1
    ("sines_48k_mono", "music", 48000, 240000, 1, 2, "sines"),
    ("sines_22k_mono_8bit", "speech", 22050, 44100, 1, 1, "sines"),
    ("chirp_48k_mono", "music", 48000, 96000, 1, 2, "chirp"),
    ("silence_8k_mono", "speech", 8000, 4000, 1, 2, "silence"),
)
SKIPPED = ("take_raw", ".hidden")  # stems the loader must skip (movenet/dataset.py:126)


def signal(kind: str, rate: int, frames: int, channels: int, seed: int) -> np.ndarray:
    """(frames, channels) float64 in (-1, 1): closed forms of t = i / rate."""
    t = np.arange(frames, dtype=np.float64) / rate
    out = np.zeros((frames, channels))
    if kind == "silence":
        return out
    for c in range(channels):
        if kind == "sines":
            # three incommensurate partials well below every Nyquist limit in play (8 kHz output, 4 kHz input)
            f0 = 97.0 + 31.0 * seed + 13.0 * c
            out[:, c] = (0.55 * np.sin(2 * np.pi * f0 * t + 0.3 * c)
                         + 0.27 * np.sin(2 * np.pi * 2.7183 * f0 * t + 1.1)
                         + 0.11 * np.sin(2 * np.pi * 5.4321 * f0 * t + 2.3 + c))
        elif kind == "chirp":
            dur = frames / rate
            out[:, c] = 0.8 * np.sin(2 * np.pi * (120.0 * t + 0.5 * (1500.0 - 120.0) / dur * t * t))
        else:
            raise ValueError(kind)
    return out


def quantise(x: np.ndarray, width: int) -> np.ndarray:
    """float (-1, 1) -> the integers a WAV of ``width`` bytes stores (8-bit: unsigned)."""
    if width == 1:
        return np.clip(np.round(x * 127.0) + 128, 0, 255).astype(np.uint8)
    if width == 2:
        return np.clip(np.round(x * 32767.0), -32768, 32767).astype("<i2")
    raise ValueError(width)


def write_wav(path: str, samples: np.ndarray, rate: int) -> None:
    """samples: (frames, channels) uint8 or int16."""
    with wave.open(path, "wb") as w:
        w.setnchannels(samples.shape[1])
        w.setsampwidth(samples.dtype.itemsize)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(samples).tobytes())


def write_float_wav(path: str, frames: int = 64, rate: int = 8000) -> None:
    """A WAVE_FORMAT_IEEE_FLOAT file (format tag 3), written by hand: ``wave`` refuses to."""
    import struct
    data = np.zeros(frames, dtype="<f4").tobytes()
    fmt = struct.pack("<HHIIHH", 3, 1, rate, rate * 4, 4, 32)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(data)) + data
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def as_pcm16(samples: np.ndarray) -> np.ndarray:
    """What the loader ships for these stored integers: int16 as stored, 8-bit as (v - 128) << 8."""
    if samples.dtype == np.uint8:
        return ((samples.astype(np.int16) - 128) << 8).astype(np.int16)
    return samples.astype(np.int16)


def write_tree(root, material=MATERIAL, valid: int = 2, skipped: bool = True) -> list:
    """Writes the tree; returns, for the train split in the loader's order (contexts sorted, then file names),
    dicts with path, context, rate, frames, channels and the (frames, channels) int16 samples as shipped."""
    root = str(root)
    clips = []
    for seed, (name, context, rate, frames, channels, width, kind) in enumerate(material):
        stored = quantise(signal(kind, rate, frames, channels, seed), width)
        d = os.path.join(root, "train", context)
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, name + ".wav")
        write_wav(path, stored, rate)
        clips.append(dict(path=path, context=context, rate=rate, frames=frames, channels=channels,
                          pcm=as_pcm16(stored), name=name))
    if skipped:
        first = clips[0]
        for stem in SKIPPED:
            write_wav(os.path.join(os.path.dirname(first["path"]), stem + ".wav"), first["pcm"][:100], first["rate"])
    for j, (name, context, rate, frames, channels, width, kind) in enumerate(material[:valid]):
        d = os.path.join(root, "valid", context)
        os.makedirs(d, exist_ok=True)
        write_wav(os.path.join(d, name + ".wav"), quantise(signal(kind, rate, frames, channels, 50 + j), width), rate)
    return sorted(clips, key=lambda c: (c["context"], os.path.basename(c["path"])))


def write_learning_tree(root, clips: int = 4, rate: int = 8000, frames: int = 16000) -> None:
    """The learning test's tree: ``clips`` short mono 16-bit sums of two sines (train), one more for valid."""
    for split, count in (("train", clips), ("valid", 1)):
        d = os.path.join(str(root), split, "tones")
        os.makedirs(d, exist_ok=True)
        for j in range(count):
            t = np.arange(frames, dtype=np.float64) / rate
            f0 = 110.0 + 20.0 * j + (7.0 if split == "valid" else 0.0)
            x = 0.6 * np.sin(2 * np.pi * f0 * t) + 0.3 * np.sin(2 * np.pi * 2.0 * f0 * t + 0.5 + j)
            write_wav(os.path.join(d, f"tone{j}.wav"), quantise(x[:, None], 2), rate)


# ---- the restatement ---------------------------------------------------------------------------------------------

def downmix_np(pcm: np.ndarray, dtype=np.float64) -> np.ndarray:
    """(frames, channels) int16 -> (frames,) mean over channels of pcm / 2^15."""
    x = pcm.astype(dtype) / dtype(32768.0)
    return x.mean(axis=1, dtype=dtype)


def resample_np(m: np.ndarray, n_out: int, dtype=np.float64, chunk: int = 8192) -> np.ndarray:
    """The whole clip ``m`` (n,) to exactly ``n_out`` frames: y[k] = sum_i m[i] h(i - k orig/new)."""
    n = int(m.shape[0])
    g = math.gcd(n, n_out)
    orig, new = n // g, n_out // g
    s64 = 0.99 * min(orig, new) / orig          # base / orig
    W = int(6.0 / s64) + 1                      # |u| < 6 needs |i - c| < 6 / s
    s, pi = dtype(s64), dtype(np.pi)
    mp = np.concatenate([np.zeros(W, dtype), m.astype(dtype), np.zeros(W + 2, dtype)])  # m[i] = 0 outside the clip
    d = np.arange(-W, W + 2, dtype=np.int64)
    y = np.empty(n_out, dtype)
    for k0 in range(0, n_out, chunk):
        k = np.arange(k0, min(n_out, k0 + chunk), dtype=np.int64)
        p = k * orig                                                  # 64-bit integers: the phase is exact
        i0 = p // new
        frac = (p - i0 * new).astype(dtype) / dtype(new)
        u = (d[None, :].astype(dtype) - frac[:, None]) * s
        with np.errstate(invalid="ignore", divide="ignore"):
            sinc = np.where(u == 0, dtype(1.0), np.sin(pi * u) / (pi * u))
        cw = np.cos(pi * u / dtype(12.0))
        h = np.where(np.abs(u) < 6, s * sinc * (cw * cw), dtype(0.0)).astype(dtype)
        taps = mp[i0[:, None] + d[None, :] + W]
        y[k] = (taps * h).sum(axis=1, dtype=dtype)
    return y


def quantise_np(y: np.ndarray, Q: int, normalize: bool, dtype=np.float64) -> np.ndarray:
    y = y.astype(dtype)
    mn, mx = y.min(), y.max()
    if normalize and mx != mn:
        y = (y - mn) / (mx - mn)
        y = y * dtype(2.0) - dtype(1.0)
    mu = dtype(Q - 1)
    z = np.sign(y) * np.log1p(mu * np.abs(y)) / np.log1p(mu)
    q = ((z + dtype(1.0)) / dtype(2.0) * mu + dtype(0.5)).astype(np.int64)
    return np.clip(q, 0, Q - 1)


def frontend_np(pcm: np.ndarray, n_out: int, Q: int, normalize: bool = True, dtype=np.float64):
    """(frames, channels) int16 -> (y (n_out,) before normalisation, class indices (n_out,) int64)."""
    y = resample_np(downmix_np(pcm, dtype), n_out, dtype)
    return y, quantise_np(y, Q, normalize, dtype)


# ---- how far a resampled sine may lie from the sine ---------------------------------------------------------------

def kernel_response(nu: np.ndarray, s: float, steps: int = 48000) -> np.ndarray:
    """H(nu) = integral of h(t) cos(2 pi nu t) dt over |t| < 6 / s (h is even), nu in cycles per INPUT sample;
    h(t) = s sinc(pi s t) cos^2(pi s t / 12).  Midpoint rule on a grid far finer than any nu used."""
    T = 6.0 / s
    t = (np.arange(steps) + 0.5) * (2 * T / steps) - T
    h = s * np.sinc(s * t) * np.cos(np.pi * s * t / 12.0) ** 2
    return (h[None, :] * np.cos(2 * np.pi * np.asarray(nu, dtype=np.float64)[:, None] * t[None, :])).sum(1) * (2 * T / steps)


def interpolation_error_bound(f: float, n: int, n_out: int, images: int = 64) -> float:
    """Bound on |y[k] - sin(2 pi f c_k + phi)| for a unit sine of ``f`` cycles per input sample, away from the
    clip's ends.  The sampled sine is the sum of the sine and its images at f + j (j != 0, cycles per input sample);
    y is that sum convolved with h, so  y = H(f) sine + sum_j H(f + j) image_j  and
        |error| <= |H(f) - 1| + sum_{j != 0} |H(f + j)|.
    The images up to ``images`` are summed; the rest is bounded by the envelope C / nu^3 of the Hann-windowed
    sinc's response, C taken from the upper half of the summed images: sum_{j > J} 2 C / j^3 <= C / J^2."""
    g = math.gcd(n, n_out)
    orig, new = n // g, n_out // g
    s = 0.99 * min(orig, new) / orig
    j = np.arange(1, images + 1, dtype=np.float64)
    near = abs(kernel_response(np.array([f]), s)[0] - 1.0)
    img = np.abs(kernel_response(np.concatenate([j - f, j + f]), s))
    upper = np.concatenate([j, j]) >= images // 2
    C = (img[upper] * np.concatenate([j - f, j + f])[upper] ** 3).max()
    return float(near + img.sum() + C / images ** 2)
