"""Float64 restatement of top-k / top-p truncation of a sampled generator step (include/movenet_hip.h,
mvn_generate_trunc): the kept set, the truncated inclusive CDF, and which steps are CLEAR -- steps whose kept set does
not hinge on the last bits of an fp32 sum or of the hardware exp.  Numpy only; every function works on the last axis
and broadcasts over the leading ones.

Tolerances.  SUM_EPS = 2^-14: the project's bound on a 256-term fp32 running sum (tests/test_model_sampling_gpu.py's
header: four times 256 x 2^-24).  The kernels compare an fp32 sum of kept weights with the fp32 product p * S, so a
step is decided by rounding only if the float64 kept set changes somewhere between p (1 - SUM_EPS) and p (1 + SUM_EPS).
TIE_EPS = 2^-18: a weight exp((l - max) / T) formed in fp32 carries the 1-2 ulp of the hardware exp and the rounding
of its argument (2^-24 |argument|, |argument| up to a few tens): two weights closer than that, relatively, may order
either way or tie in fp32."""
from __future__ import annotations

import numpy as np

SUM_EPS = 2.0 ** -14
TIE_EPS = 2.0 ** -18


def model_weights(logits, temperature: float) -> np.ndarray:
    """exp((l - max l) / T): the unnormalised weights of the "model" rule."""
    z = np.asarray(logits, dtype=np.float64)
    return np.exp((z - z.max(axis=-1, keepdims=True)) / float(temperature))


def reference_weights(logits, temperature: float) -> np.ndarray:
    """The "reference" rule's weights, unnormalised: exp(x - max x) with x = softmax(l) / T."""
    x = model_weights(logits, 1.0)
    x = x / x.sum(axis=-1, keepdims=True) / float(temperature)
    return np.exp(x - x.max(axis=-1, keepdims=True))


def _desc(w):
    return -np.sort(-w, axis=-1)


def thresholds(w, top_k: int = 0, top_p: float = 1.0):
    """(theta_k, theta_p), each (..., 1): class q is kept iff w_q >= max(theta_k, theta_p).  theta_k: the top_k-th
    largest weight (0 where top-k is off: top_k = 0 or >= Q).  theta_p: the largest weight value v for which the kept
    weights >= v sum to at least top_p * S, S = the sum of what top-k kept (0 where top_p >= 1)."""
    w = np.asarray(w, dtype=np.float64)
    Q = w.shape[-1]
    zero = np.zeros(w.shape[:-1] + (1,))
    theta_k = _desc(w)[..., top_k - 1:top_k] if 0 < top_k < Q else zero
    if top_p >= 1.0:
        return theta_k, zero
    ws = _desc(np.where(w >= theta_k, w, 0.0))
    cs = np.cumsum(ws, axis=-1)
    # descending, the first prefix that reaches p S ends inside the tie group of theta_p: every larger VALUE lies
    # wholly in front of it and sums to less, and the whole group of this value sums to at least this prefix
    first = (cs >= top_p * cs[..., -1:]).argmax(axis=-1)
    return theta_k, np.take_along_axis(ws, first[..., None], axis=-1)


def kept_set(w, top_k: int = 0, top_p: float = 1.0, tie: float = 0.0) -> np.ndarray:
    """Boolean (..., Q).  ``tie`` > 0 also keeps the classes within that relative distance below the threshold."""
    w = np.asarray(w, dtype=np.float64)
    theta_k, theta_p = thresholds(w, top_k, top_p)
    return w >= np.maximum(theta_k, theta_p) * (1.0 - tie)


def wide_kept_set(w, top_k: int = 0, top_p: float = 1.0) -> np.ndarray:
    """What a correct kernel may ever keep: the set for p (1 + SUM_EPS), near-ties (TIE_EPS) at the threshold kept."""
    return kept_set(w, top_k, min(1.0, top_p * (1.0 + SUM_EPS)), tie=TIE_EPS)


def truncated_cdf(w, kept) -> np.ndarray:
    """Inclusive CDF of the weights with the dropped classes zeroed; exactly 1 from the last kept class on."""
    c = np.cumsum(np.where(kept, np.asarray(w, dtype=np.float64), 0.0), axis=-1)
    return c / c[..., -1:]


def _gap_below(ws, idx):
    """Relative distance between the sorted (descending) weight at ``idx`` (...,) and the next one; inf at the end."""
    Q = ws.shape[-1]
    a = np.take_along_axis(ws, idx[..., None], axis=-1)[..., 0]
    b = np.take_along_axis(ws, np.minimum(idx + 1, Q - 1)[..., None], axis=-1)[..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((idx + 1 < Q) & (a > 0), (a - b) / a, np.inf)


def unclear(w, top_k: int = 0, top_p: float = 1.0):
    """(unclear_k, unclear_p), boolean (...,): steps whose kept set a correct fp32 kernel may form differently.
    top-k: the k-th and (k + 1)-th largest weights differ by less than TIE_EPS relative.  top-p: the kept set differs
    between p (1 - SUM_EPS) and p (1 + SUM_EPS), or the threshold weight and the next smaller weight (among what top-k
    kept) differ by less than TIE_EPS relative."""
    w = np.asarray(w, dtype=np.float64)
    Q = w.shape[-1]
    none = np.zeros(w.shape[:-1], dtype=bool)
    uk, up = none, none
    if 0 < top_k < Q:
        uk = _gap_below(_desc(w), np.full(w.shape[:-1], top_k - 1)) < TIE_EPS
    if top_p < 1.0:
        lo = kept_set(w, top_k, top_p * (1.0 - SUM_EPS))
        hi = kept_set(w, top_k, min(1.0, top_p * (1.0 + SUM_EPS)))
        theta_k, theta_p = thresholds(w, top_k, top_p)
        ws = _desc(np.where(w >= theta_k, w, 0.0))
        last = (ws >= theta_p).sum(axis=-1) - 1  # the last entry of the threshold's tie group
        up = (lo != hi).any(axis=-1) | (_gap_below(ws, last) < TIE_EPS)
    return uk, up
