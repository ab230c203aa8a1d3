"""The two F0 conditioning channels of DESIGN 4.5j restated in numpy float64 (include/movenet_hip.h:
mvn_pitch_features).  The period track is taken as given -- the fp32 values the kernel reads, ``rate`` and ``f_ref`` as
the floats it is handed -- and everything after that is float64: no rounding of lf, of the weight a or of the lerp.
Shared by the host and GPU tests; not a test module itself."""
import numpy as np

RATE, F_MIN, F_MAX = 8000.0, 60.0, 500.0
F_REF = float(np.sqrt(F_MIN * F_MAX))
CHUNK = 256  # ops.PITCH_FEATURES_CHUNK (the GPU test asserts they agree)


def voiced_of(period):
    with np.errstate(invalid="ignore"):
        return np.asarray(period) > 0  # (NaN and negative values: unvoiced)


def log_f0(period, rate, f_ref):
    """log2(rate / (period f_ref)) of voiced periods, in float64 from the float32 rate and f_ref."""
    r, f = float(np.float32(rate)), float(np.float32(f_ref))
    return np.log2(r / (np.asarray(period, dtype=np.float64) * f))


def neighbours(voiced):
    """(prev, next) of one row: the nearest voiced frame at or below / at or above each frame, -1 / F where none."""
    F = len(voiced)
    j = np.arange(F)
    prev = np.maximum.accumulate(np.where(voiced, j, -1))
    nxt = np.minimum.accumulate(np.where(voiced, j, F)[::-1])[::-1]
    return prev, nxt


def features(period, rate=RATE, f_ref=F_REF, shift=None):
    """(B, F) periods -> (B, 2, F) float64: the continuous log-F0 (plus ``shift[b]``) and the voiced flag."""
    period = np.atleast_2d(np.asarray(period))
    B, F = period.shape
    out = np.zeros((B, 2, F), dtype=np.float64)
    shift = np.zeros(B) if shift is None else np.broadcast_to(np.asarray(shift, dtype=np.float64), (B,))
    for b in range(B):
        v = voiced_of(period[b])
        out[b, 1] = v
        if not v.any():
            out[b, 0] = shift[b]
            continue
        lf = np.zeros(F)
        lf[v] = log_f0(period[b][v], rate, f_ref)
        prev, nxt = neighbours(v)
        for j in np.nonzero(~v)[0]:
            p, n = prev[j], nxt[j]
            if p < 0:
                lf[j] = lf[n]
            elif n >= F:
                lf[j] = lf[p]
            else:
                a = (j - p) / (n - p)
                lf[j] = a * lf[n] + (1.0 - a) * lf[p]
        out[b, 0] = lf + shift[b]
    return out


def ulp32(x):
    """The spacing of float32 at |x| (of the float32 nearest to it)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


# |kernel - reference| of an interpolated frame, in ulps of L = max(|lf[p]|, |lf[n]|) (ulp32(L) >= 2^-24 L):
#   1  the neighbours: each is the double expression rounded once (half an ulp, plus the device log2's own error far
#      below that: "1 ulp off"), and they enter with weights a and 1 - a that sum to 1
#   2  a = fl((j - p) / (n - p)) is off by at most 2^-24 a <= 2^-24 and multiplies lf[n] - lf[p], at most 2 L
#   1  fl(1 - a), relative 2^-24 on a factor of lf[p]
#   1  fl((1 - a) lf[p])
#   1  the fma's one rounding of a result of magnitude at most L
# Second-order terms are below 2^-24 of these and inside the halves that 1, and the last line, leave unused.
LERP_ULPS = 6.0


def tolerance(period, ref):
    """tol (B, F) for the log-F0 channel of ``features(period)`` without a shift: 1 ulp of the reference on a voiced
    frame and on a frame that holds a voiced frame's value, LERP_ULPS ulps of L on an interpolated one, 0 in a row
    without a voiced frame."""
    period = np.atleast_2d(np.asarray(period))
    tol = np.zeros(period.shape)
    for b in range(period.shape[0]):
        v = voiced_of(period[b])
        if not v.any():
            continue
        prev, nxt = neighbours(v)
        F = len(v)
        lf = ref[b, 0]
        for j in range(F):
            p, n = prev[j], nxt[j]
            if v[j] or p < 0 or n >= F:
                tol[b, j] = ulp32(lf[j])
            else:
                tol[b, j] = LERP_ULPS * ulp32(max(abs(lf[p]), abs(lf[n])))
    return tol


def interpolated(period):
    """(B, F) bool: the unvoiced frames with a voiced frame on both sides."""
    period = np.atleast_2d(np.asarray(period))
    out = np.zeros(period.shape, dtype=bool)
    for b in range(period.shape[0]):
        v = voiced_of(period[b])
        prev, nxt = neighbours(v)
        out[b] = ~v & (prev >= 0) & (nxt < len(v))
    return out


# ---- the planted tracks the GPU test runs ------------------------------------------------------------------------------
def _voiced_row(F, seed):
    """A fully voiced row: periods between RATE / F_MAX and RATE / F_MIN samples, with fractions."""
    rng = np.random.default_rng([11, seed])
    return rng.uniform(RATE / F_MAX, RATE / F_MIN, F)


def _with_gaps(F, seed, gaps):
    row = _voiced_row(F, seed)
    for lo, hi in gaps:  # frames [lo, hi) unvoiced
        row[lo:hi] = 0.0
    return row


def cases():
    """name -> (B, F) float32 planted period tracks."""
    C, F3 = CHUNK, CHUNK * 5 // 2  # (2.5 chunks)
    out = {
        "one_frame": np.array([[37.25], [0.0]]),
        "two_frames": np.array([[37.25, 0.0], [0.0, 51.5], [0.0, 0.0], [20.0, 90.5]]),
        "unvoiced_beside_voiced": np.stack([np.zeros(70), _voiced_row(70, 0)]),
        "edges_and_wave_boundary": np.stack([
            _with_gaps(130, 1, [(0, 9)]), _with_gaps(130, 2, [(117, 130)]), _with_gaps(130, 3, [(0, 5), (100, 130)]),
            _with_gaps(130, 4, [(40, 63)]), _with_gaps(130, 5, [(40, 64)]), _with_gaps(130, 6, [(40, 65)]),
            _with_gaps(130, 7, [(63, 70)]), _with_gaps(130, 8, [(64, 70)]), _with_gaps(130, 9, [(65, 70)])]),
        "chunk_boundary": np.stack(
            [_with_gaps(F3, 20 + i, [(k - 30, k)]) for i, k in enumerate((C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1))]
            + [_with_gaps(F3, 30 + i, [(k, k + 30)]) for i, k in enumerate((C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1))]
            + [_with_gaps(F3, 40, [(0, C)]), _with_gaps(F3, 41, [(2 * C, F3)]), _with_gaps(F3, 42, [(C, 2 * C)])]),
        "long_gap": np.stack([_with_gaps(F3, 50, [(0, 3), (4, F3 - 200), (F3 - 199, F3)]),
                              _with_gaps(F3, 51, [(0, F3 - 1)]), _with_gaps(F3, 52, [(1, F3)])]),
    }
    odd = _with_gaps(F3, 60, [(10, 40), (300, 330)])
    odd[12], odd[20], odd[310] = np.nan, -44.0, -np.inf  # inside the gaps ...
    odd[100], odd[101], odd[500] = np.nan, -3.5, np.nan  # ... and single frames of their own
    out["nan_and_negative"] = np.stack([odd, np.full(F3, np.nan), np.full(F3, -1.0)])
    return {k: v.astype(np.float32) for k, v in out.items()}
