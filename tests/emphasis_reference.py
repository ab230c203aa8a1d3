"""Float64 restatement of pre-emphasis (mvn_audio_frontend_emph) and of the de-emphasising PCM conversion
(mvn_pcm16_deemph_chunk), written from the definitions in include/movenet_hip.h alone -- none of the library's code is
used.  The coefficient is the float32 value the kernels take, widened."""
import numpy as np


def coefficient(a) -> np.float64:
    return np.float64(np.float32(a))


def preemphasise(vn, a) -> np.ndarray:
    """e[k] = (vn[k] - a vn[k-1]) / (1 + a) along the last axis, vn[-1] = 0, in float64."""
    vn = np.asarray(vn, dtype=np.float64)
    a = coefficient(a)
    prev = np.concatenate([np.zeros_like(vn[..., :1]), vn[..., :-1]], axis=-1)
    return (vn - a * prev) / (1.0 + a)


def deemphasise(e, a, y0=None) -> np.ndarray:
    """The inverse filter in float64: y[t] = (1 + a) e[t] + a y[t-1] along the last axis, y[-1] = y0 (default 0)."""
    e = np.asarray(e, dtype=np.float64)
    a = coefficient(a)
    y = np.zeros(e.shape[:-1]) if y0 is None else np.array(y0, dtype=np.float64)
    out = np.empty_like(e)
    for t in range(e.shape[-1]):
        y = (1.0 + a) * e[..., t] + a * y
        out[..., t] = y
    return out


def deemph_pcm16(x_float32, a, y0=None):
    """The sequential loop of mvn_pcm16_deemph_chunk over (rows, T) float32 decoded samples, vectorised over rows:
    y = ((1 + a) x) + (a y_prev), two products and one sum, each a float64 operation of its own (numpy fuses nothing);
    pcm = rint(clip(y, -1, 1) 32767).  Returns (pcm int16 (rows, T), final state float64 (rows,))."""
    x = np.asarray(x_float32)
    assert x.dtype == np.float32 and x.ndim == 2, (x.dtype, x.shape)
    x = x.astype(np.float64)
    a = coefficient(a)
    gain = np.float64(1.0) + a
    y = np.zeros(x.shape[0], dtype=np.float64) if y0 is None else np.array(y0, dtype=np.float64)
    pcm = np.empty(x.shape, dtype=np.int16)
    for t in range(x.shape[1]):
        y = (gain * x[:, t]) + (a * y)
        pcm[:, t] = np.rint(np.clip(y, -1.0, 1.0) * 32767.0).astype(np.int16)
    return pcm, y


def self_check(seed: int = 0) -> float:
    """max |deemphasise(preemphasise(v)) - v| over random rows and both coefficients the tests use, in float64."""
    rng = np.random.default_rng(seed)
    worst = 0.0
    for a in (0.97, 0.5):
        v = rng.uniform(-1.0, 1.0, size=(4, 3000))
        worst = max(worst, float(np.abs(deemphasise(preemphasise(v, a), a) - v).max()))
    return worst
