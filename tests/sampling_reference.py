"""Float64 / exact-integer restatement of what a sampled generator step computes under the "model" rule
(include/movenet_hip.h, MVN_SAMPLE_MODEL): the Philox uniform of (seed, time, sequence) and the inverse CDF of
softmax(logits / T).  Numpy only; shared by the model-sampling tests."""
from __future__ import annotations

import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox_uniform(seed: int, c0, c1) -> np.ndarray:
    """csrc/common.h philox_uniform: ten Philox4x32 rounds on the counter (c0, c1, 0x6d766e31, 0) under the key
    (seed low word, seed high word); the result is (c[0] >> 8) / 2^24 -- a multiple of 2^-24 in [0, 1), exact in
    float64.  ``c0`` / ``c1`` broadcast against each other (generators: c0 = the time u drawn for, c1 = the
    sequence's index in its launch)."""
    c0, c1 = np.broadcast_arrays(np.asarray(c0, dtype=np.uint64), np.asarray(c1, dtype=np.uint64))
    c = [c0 & _MASK, c1 & _MASK, np.full(c0.shape, 0x6D766E31, dtype=np.uint64), np.zeros(c0.shape, dtype=np.uint64)]
    seed = int(seed) & (2 ** 64 - 1)
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]          # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> _S32, p0 & _MASK, p1 >> _S32, p1 & _MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return (c[0] >> np.uint64(8)).astype(np.float64) / 16777216.0


def model_cdf(logits, temperature: float) -> np.ndarray:
    """Inclusive CDF over the last axis of softmax(logits / T) in float64 (the last entry is exactly 1)."""
    z = np.asarray(logits, dtype=np.float64)
    w = np.cumsum(np.exp((z - z.max(axis=-1, keepdims=True)) / float(temperature)), axis=-1)
    return w / w[..., -1:]


def model_probs(logits, temperature: float) -> np.ndarray:
    z = np.asarray(logits, dtype=np.float64)
    e = np.exp((z - z.max(axis=-1, keepdims=True)) / float(temperature))
    return e / e.sum(axis=-1, keepdims=True)


def inverse_cdf_picks(cdf: np.ndarray, uniform: np.ndarray) -> np.ndarray:
    """The smallest class whose CDF exceeds the uniform (total = 1), Q - 1 if none does."""
    hit = cdf > uniform[..., None]
    return np.where(hit.any(axis=-1), hit.argmax(axis=-1), cdf.shape[-1] - 1)


def band_excess(picks: np.ndarray, cdf: np.ndarray, uniform: np.ndarray) -> np.ndarray:
    """How far each draw lies outside the float64 band of its pick, cdf[pick - 1] <= uniform < cdf[pick]
    (cdf[-1] = 0): 0 inside the band, the distance to the nearer edge outside."""
    picks = picks.astype(np.int64)
    hi = np.take_along_axis(cdf, picks[..., None], axis=-1)[..., 0]
    lo = np.where(picks > 0, np.take_along_axis(cdf, np.maximum(picks - 1, 0)[..., None], axis=-1)[..., 0], 0.0)
    return np.maximum(np.maximum(lo - uniform, uniform - hi), 0.0)
