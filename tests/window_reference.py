"""The by-rate resample of a WINDOW of a file, restated in numpy (a helper, not a test).

``resample_window_np`` evaluates only the requested columns [out_first, out_first + n_out) of the resample of a whole
file from ``rate_in`` to ``rate_out`` -- the formula of ``wav_material.resample_np`` with (orig, new) taken from the
rates instead of from (frames, n_out), and the global output index in place of the local one -- from the span of the
file's channel mean that those columns' taps reach.  In float64 it is the definition the kernel is held to; in float32
the same formula at the kernel's precision, which the kernel's tolerance is derived from.  ``file_frames`` may be far
larger than the span: nothing outside the span is looked at, and a tap outside it that lies inside the file is an
error of the caller's plan.
"""
from __future__ import annotations

import math

import numpy as np


def geometry(rate_in: int, rate_out: int) -> tuple:
    """(orig, new, s, W): the reduced ratio, the tap argument's scale and the taps' reach i0 - W .. i0 + W + 1."""
    g = math.gcd(rate_in, rate_out)
    orig, new = rate_in // g, rate_out // g
    s = 0.99 * min(orig, new) / orig
    return orig, new, s, int(6.0 / s) + 1


def n_file(file_frames: int, rate_in: int, rate_out: int) -> int:
    orig, new, _, _ = geometry(rate_in, rate_out)
    return -(-file_frames * new // orig)


def tap_range(file_frames: int, rate_in: int, rate_out: int, out_first: int, n_out: int) -> tuple:
    """(first, last) source frame the columns' taps reach, clipped to the file."""
    orig, new, _, W = geometry(rate_in, rate_out)
    return (max(0, out_first * orig // new - W),
            min(file_frames - 1, (out_first + n_out - 1) * orig // new + W + 1))


def resample_window_np(m_span: np.ndarray, span_first: int, file_frames: int, rate_in: int, rate_out: int,
                       out_first: int, n_out: int, dtype=np.float64, chunk: int = 1024) -> np.ndarray:
    """``m_span``: the file's channel mean on [span_first, span_first + len(m_span)).  Returns y (n_out,)."""
    orig, new, s64, W = geometry(rate_in, rate_out)
    assert 0 <= out_first and out_first + n_out <= n_file(file_frames, rate_in, rate_out)
    s, pi = dtype(s64), dtype(np.pi)
    m = np.concatenate([m_span.astype(dtype), np.zeros(1, dtype)])       # [-1]: a tap outside the file
    d = np.arange(-W, W + 2, dtype=np.int64)
    y = np.empty(n_out, dtype)
    for k0 in range(0, n_out, chunk):
        j = out_first + np.arange(k0, min(n_out, k0 + chunk), dtype=np.int64)
        p = j * orig                                                     # 64-bit integers: the phase is exact
        i0 = p // new
        frac = (p - i0 * new).astype(dtype) / dtype(new)
        u = (d[None, :].astype(dtype) - frac[:, None]) * s
        with np.errstate(invalid="ignore", divide="ignore"):
            sinc = np.where(u == 0, dtype(1.0), np.sin(pi * u) / (pi * u))
        cw = np.cos(pi * u / dtype(12.0))
        h = np.where(np.abs(u) < 6, s * sinc * (cw * cw), dtype(0.0)).astype(dtype)
        at = i0[:, None] + d[None, :]
        inside = (at >= 0) & (at < file_frames)
        rel = at - span_first
        assert bool(((rel >= 0) & (rel < len(m_span)))[inside].all()), "the span does not cover the window's taps"
        taps = m[np.where(inside, rel, -1)]
        y[k0:k0 + len(j)] = (taps * h).sum(axis=1, dtype=dtype)
    return y
