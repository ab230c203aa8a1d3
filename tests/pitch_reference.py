"""The pitch tracker and the pitch-track distance of DESIGN 4.5i restated in numpy float64 (include/movenet_hip.h:
mvn_pitch_frames, mvn_pitch_distance).  The signal is taken as given -- the fp32 samples the kernel reads -- and
everything after it is float64.  Shared by the host and GPU tests; not a test module itself."""
import numpy as np


def frames_of(n_samples: int, hop: int) -> int:
    return n_samples // hop + 1


def frame_signal(x, j: int, win: int, hop: int, tau_max: int):
    """The L = win + tau_max samples of frame j of one row, zeros outside the row."""
    L = win + tau_max
    s = j * hop - L // 2
    out = np.zeros(L, dtype=np.float64)
    lo, hi = max(s, 0), min(s + L, len(x))
    if hi > lo:
        out[lo - s:hi - s] = np.asarray(x[lo:hi], dtype=np.float64)
    return out


def cmnd_of_frame(frame, win: int, tau_max: int):
    """c(0 .. tau_max) of one frame: the cumulative-mean-normalised difference function."""
    d = np.zeros(tau_max + 1, dtype=np.float64)
    head = frame[:win]
    for tau in range(1, tau_max + 1):
        diff = head - frame[tau:tau + win]
        d[tau] = np.dot(diff, diff)
    run = np.cumsum(d[1:])
    c = np.ones(tau_max + 1, dtype=np.float64)
    live = run > 0
    c[1:][live] = d[1:][live] * np.arange(1, tau_max + 1)[live] / run[live]
    return c


def pick(c, tau_min: int, tau_max: int, threshold: float):
    """(voiced, tau_star, period, aper) of one frame from its c."""
    below = [t for t in range(tau_min, tau_max + 1) if c[t] < threshold]
    if below:
        voiced, t = True, below[0]
        while t + 1 <= tau_max and c[t + 1] < c[t]:
            t += 1
    else:
        voiced, t = False, tau_min + int(np.argmin(c[tau_min:tau_max + 1]))  # (argmin: the first of equal minima)
    period = float(t)
    if t - 1 >= 1 and t + 1 <= tau_max and c[t] <= c[t - 1] and c[t] <= c[t + 1]:
        den = 2.0 * (c[t - 1] - 2.0 * c[t] + c[t + 1])
        if den != 0.0:
            period += (c[t - 1] - c[t + 1]) / den
    return voiced, t, period if voiced else 0.0, float(c[t])


def pick_is_safe(c, tol, tau_min: int, tau_max: int, threshold: float) -> bool:
    """Whether a c that differs from ``c`` by at most ``tol`` element-wise (``tol``: an array like c) must lead to the
    same voiced flag and the same tau*: no c of the range within tol of the threshold, and every pair the walk or the
    argmin compares further apart than the two tolerances together."""
    def close(i, k):  # (two values that carry no error compare as they do here, equal ones included)
        return tol[i] + tol[k] > 0 and abs(c[i] - c[k]) <= tol[i] + tol[k]
    r = slice(tau_min, tau_max + 1)
    if np.any(np.abs(c[r] - threshold) <= tol[r]):
        return False
    voiced, t, _, _ = pick(c, tau_min, tau_max, threshold)
    if voiced:
        first = next(k for k in range(tau_min, tau_max + 1) if c[k] < threshold)
        # the comparisons c[k + 1] < c[k] the walk made, the one that stopped it too
        if any(close(k + 1, k) for k in range(first, min(t + 1, tau_max))):
            return False
    elif any(close(k, t) for k in range(tau_min, tau_max + 1) if k != t):
        return False
    # the refinement's own test: c[t] against the neighbours it has
    return not any(close(k, t) for k in (t - 1, t + 1) if 1 <= k <= tau_max)


def period_bound(c, tol, t: int, tau_max: int):
    """How far the refined period of a c within ``tol`` of ``c`` may lie from this c's, both picked at tau* = t where
    the refinement applies to both: with N = c0 - c2, D = 2 (c0 - 2 c1 + c2) and the offset o = N / D, the inputs move
    N by at most eN = tol0 + tol2 and D by at most eD = 2 (tol0 + 2 tol1 + tol2); the fp32 evaluation adds a rounding
    of 2^-24 per operation: 2^-23 (|c0| + |c2|) to eN and 2^-22 (|c0| + 2 |c1| + |c2|) to eD.  Then
        |o' - o| <= (eN + |o| eD) / (|D| - eD),
    plus 2^-23 (t + 1) for the division and the final sum.  None where eD >= |D| (no bound: the frame is not safe)."""
    if not (t - 1 >= 1 and t + 1 <= tau_max and c[t] <= c[t - 1] and c[t] <= c[t + 1]):
        return 2.0 ** -23 * (t + 1)
    c0, c1, c2 = c[t - 1], c[t], c[t + 1]
    n, d = c0 - c2, 2.0 * (c0 - 2.0 * c1 + c2)
    if d == 0.0:
        return None if tol[t - 1] + tol[t] + tol[t + 1] > 0 else 2.0 ** -23 * (t + 1)
    en = tol[t - 1] + tol[t + 1] + 2.0 ** -23 * (abs(c0) + abs(c2))
    ed = 2.0 * (tol[t - 1] + 2.0 * tol[t] + tol[t + 1]) + 2.0 ** -22 * (abs(c0) + 2.0 * abs(c1) + abs(c2))
    if ed >= abs(d):
        return None
    return (en + abs(n / d) * ed) / (abs(d) - ed) + 2.0 ** -23 * (t + 1)


def track(x, win: int, hop: int, tau_min: int, tau_max: int, threshold: float):
    """(B, T) samples -> dict of cmnd (B, F, tau_max + 1), voiced (B, F) bool, tau (B, F) int, period, aper (B, F)."""
    x = np.atleast_2d(np.asarray(x))
    B, T = x.shape
    F = frames_of(T, hop)
    out = {"cmnd": np.zeros((B, F, tau_max + 1)), "voiced": np.zeros((B, F), dtype=bool),
           "tau": np.zeros((B, F), dtype=np.int64), "period": np.zeros((B, F)), "aper": np.zeros((B, F))}
    for b in range(B):
        for j in range(F):
            c = cmnd_of_frame(frame_signal(x[b], j, win, hop, tau_max), win, tau_max)
            out["cmnd"][b, j] = c
            out["voiced"][b, j], out["tau"][b, j], out["period"][b, j], out["aper"][b, j] = pick(c, tau_min, tau_max,
                                                                                                 threshold)
    return out


def mu_law_decode(index, classes: int):
    """The mu-law expansion in float64 (0 for an index outside [0, classes))."""
    index = np.asarray(index, dtype=np.int64)
    mu = classes - 1.0
    y = index / mu * 2.0 - 1.0
    x = np.sign(y) * (np.exp(np.abs(y) * np.log1p(mu)) - 1.0) / mu
    return np.where((index < 0) | (index >= classes), 0.0, x)


def distance(period_a, period_b, first, count, gross_ratio: float = 0.2):
    """(rmse_cents (B,), counts (B, 4): both, vuv, gross, clamped count) of two (B, F) period tracks."""
    a, b = np.asarray(period_a, dtype=np.float64), np.asarray(period_b, dtype=np.float64)
    B, F = a.shape
    rmse, counts = np.zeros(B), np.zeros((B, 4), dtype=np.int64)
    for s in range(B):
        lo = min(max(int(first[s]), 0), F)
        hi = min(max(int(first[s]) + int(count[s]), lo), F)
        pa, pb = a[s, lo:hi], b[s, lo:hi]
        with np.errstate(invalid="ignore"):
            va, vb = pa > 0, pb > 0
        both = va & vb
        e = 1200.0 * np.log2(pb[both] / pa[both])
        counts[s] = (both.sum(), (va != vb).sum(), (np.abs(pa[both] / pb[both] - 1.0) > gross_ratio).sum(), hi - lo)
        rmse[s] = np.sqrt(np.sum(e * e) / both.sum()) if both.any() else 0.0
    return rmse, counts


# ---- the inputs the GPU tests and the host test of the seeds share -----------------------------------------------------
SETTINGS = [(64, 16, 4, 40), (200, 50, 3, 150), (512, 128, 20, 300)]  # (win, hop, tau_min, tau_max)
ROWS, SAMPLES, THRESHOLD = 3, 2000, 0.15
SEEDS = (2, 15, 0)  # one per row: the first for which the reference alone leaves at most 5 % of a row's frames unsafe


def make_row(kind: int, tau_min: int, tau_max: int, seed: int):
    """One row of ``make_rows`` in float64, from a generator of its own."""
    rng = np.random.default_rng([kind, seed])
    t = np.arange(SAMPLES, dtype=np.float64)
    if kind == 0:  # a two-harmonic tone of a non-integer period (its octave below is in range too) plus noise
        period = 0.5 * (tau_min + tau_max) * 0.61 + 0.37 + 0.1 * rng.random()
        return 0.6 * np.sin(2 * np.pi * t / period + rng.random()) + 0.25 * np.sin(4 * np.pi * t / period + 0.4) \
            + 0.01 * rng.standard_normal(SAMPLES)
    if kind == 1:  # a chirp with twelve harmonics whose period crosses the lag range from below tau_min to above tau_max
        p = np.linspace(0.6 * tau_min + 1.0, 1.3 * tau_max, SAMPLES)  # the period, sample by sample
        phase = 2 * np.pi * (np.cumsum(1.0 / p) + rng.random())
        chirp = sum(np.sin(k * phase + 0.3 * k) / k for k in range(1, 13))
        return 0.7 * chirp / np.abs(chirp).max() + 0.01 * rng.standard_normal(SAMPLES)
    # half constant, half noise.  The constant is the padding's 0: a step from the padding to another level gives the
    # edge frames a c that falls towards 1 by ~1e-4 per lag at tau_max, every one of them inside the tolerance of its
    # neighbour (the planted constant of test_planted_known_answers is 0.25)
    cut = SAMPLES // 2 + int(rng.integers(-60, 61))
    return np.concatenate([np.zeros(cut), 0.3 * rng.standard_normal(SAMPLES - cut)])


def make_rows(tau_min: int, tau_max: int, seeds=SEEDS):
    """(3, 2000) float32: a two-harmonic tone of a non-integer period plus seeded noise; a chirp whose period crosses
    the lag range; a row that is half constant and half noise."""
    return np.stack([make_row(k, tau_min, tau_max, s) for k, s in enumerate(seeds)]).astype(np.float32)


def cmnd_rtol(win: int, tau_max: int) -> float:
    """4 (win + tau_max) 2^-24: twice the forward-error bound of the two fp32 sums of non-negative terms behind c --
    d(tau), win terms, and its running sum, at most tau_max terms, each with relative error at most (terms) 2^-24."""
    return 4.0 * (win + tau_max) * 2.0 ** -24


# 4 x the largest |c_kernel - c_float64| measured on an MI355X over the three SETTINGS on make_rows: 3.333e-06,
# 6.097e-06 and 8.733e-06 (c reaches ~7 there, the largest relative deviation was 1.4e-06).  The factor
# allows for another summation order.
CMND_ATOL = 4.0 * 8.733e-6


def cmnd_tolerance(x, cmnd, win: int, hop: int, tau_max: int, atol: float = CMND_ATOL):
    """tol like cmnd: rtol c + atol, and 0 where c carries no error: c(0), and every lag up to which the frame's first
    win + tau samples are all equal -- each difference behind d(1 .. tau) is then an exact 0 in fp32 as in float64, the
    running sum is 0 and c is exactly 1 in both (a constant frame: all of its lags)."""
    tol = cmnd_rtol(win, tau_max) * np.abs(cmnd) + atol
    tol[:, :, 0] = 0.0
    for b in range(cmnd.shape[0]):
        for j in range(cmnd.shape[1]):
            f = frame_signal(x[b], j, win, hop, tau_max)
            differs = np.nonzero(f != f[0])[0]
            equal = len(f) if len(differs) == 0 else int(differs[0])  # the frame's first `equal` samples are one value
            if equal > win:
                tol[b, j, 1:equal - win + 1] = 0.0
    return tol


def safe_frames(ref, tol, tau_min: int, tau_max: int, threshold: float):
    """(safe (B, F) bool, bound (B, F)): the frames whose decision any c within tol of the reference's shares, and the
    period bound of each (``period_bound``; a frame without one is not safe)."""
    B, F = ref["voiced"].shape
    safe, bound = np.zeros((B, F), dtype=bool), np.zeros((B, F))
    for b in range(B):
        for j in range(F):
            c, t = ref["cmnd"][b, j], int(ref["tau"][b, j])
            pb = period_bound(c, tol[b, j], t, tau_max)
            safe[b, j] = pb is not None and pick_is_safe(c, tol[b, j], tau_min, tau_max, threshold)
            bound[b, j] = pb if pb is not None else np.inf
    return safe, bound
