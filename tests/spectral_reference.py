"""The float64 numpy restatement of the spectral distance (a helper, not a test): ``feature_distance`` and
``distance_frame_span`` as DESIGN 4.5g defines them.  Plain loops and numpy sums; nothing of the package is used."""
from __future__ import annotations

import math

import numpy as np

DB_PER_NAT = 10.0 / math.log(10.0)


def feature_distance(a, b, first=None, count=None):
    """a, b: (B, M, F) arrays.  Returns (lsd_db (B,), l1 (B,), per_frame (B, F)), all float64; only the frames
    [first_b, first_b + count_b) of sequence b are looked at, an empty span gives 0.0."""
    a, b = np.asarray(a), np.asarray(b)
    B, M, F = a.shape
    first = [0] * B if first is None else [int(v) for v in first]
    count = [F - f for f in first] if count is None else [int(v) for v in count]
    lsd, l1, per_frame = np.zeros(B), np.zeros(B), np.zeros((B, F))
    for s in range(B):
        f0, n = first[s], count[s]
        assert 0 <= f0 and 0 <= n and f0 + n <= F
        if n == 0:
            continue
        d = a[s, :, f0:f0 + n].astype(np.float64) - b[s, :, f0:f0 + n].astype(np.float64)
        rms = np.sqrt((d * d).sum(axis=0) / M)
        lsd[s] = DB_PER_NAT * (rms.sum() / n)
        l1[s] = np.abs(d).sum() / (M * n)
        per_frame[s, f0:f0 + n] = rms * DB_PER_NAT
    return lsd, l1, per_frame


def distance_frame_span(lengths, T, n_fft, hop, skip=0):
    """(first, count) lists: frame f covers samples [f hop - h, f hop - h + n_fft), h = n_fft // 2, and counts when
    that window lies inside [skip, len_b).  Found by trying every frame, not by the closed form."""
    h, F = n_fft // 2, T // hop + 1
    first, count = [], []
    for n in lengths:
        inside = [f for f in range(F) if f * hop - h >= skip and f * hop - h + n_fft <= n]
        first.append(-((-(skip + h)) // hop))
        count.append(len(inside))
        assert not inside or (inside[0] == first[-1] and inside == list(range(inside[0], inside[-1] + 1)))
    return first, count
