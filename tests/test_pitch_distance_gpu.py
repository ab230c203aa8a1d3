"""GPU: mvn_pitch_distance through ``ops.pitch_distance`` against float64 numpy (tests/pitch_reference.py)
on hand-built period tracks: all unvoiced, a known cents offset, planted voicing flips and an octave error, frames
outside the span poisoned with NaN, an empty span."""
import math

import numpy as np
import pytest
import torch

import pitch_reference as R
from helpers import DEV
from movenet_amd import ops

pytestmark = pytest.mark.gpu
F = 150  # more than one pass of the wave's 64 lanes


def _run(a, b, first=None, count=None, **kw):
    out = ops.pitch_distance(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), first, count, **kw)
    assert out["f0_rmse_cents"].dtype == torch.float64 and out["voiced_frames"].dtype == torch.int32
    return out["f0_rmse_cents"].cpu().numpy(), np.stack([out[k].cpu().numpy() for k in
                                                       ("voiced_frames", "vuv_errors", "gross_errors", "frames")], axis=1)


def _tracks(seed=0):
    rng = np.random.default_rng(seed)
    return (40.0 + 60.0 * rng.random((3, F))).astype(np.float32)


def test_all_unvoiced_gives_zeros():
    z = np.zeros((2, F), np.float32)
    rmse, counts = _run(z, z)
    assert rmse.tolist() == [0.0, 0.0] and counts.tolist() == [[0, 0, 0, F]] * 2


def test_a_known_offset_in_cents():
    a = _tracks()
    for cents in (100.0, -35.0, 3.0):
        b = (a.astype(np.float64) * 2.0 ** (cents / 1200.0)).astype(np.float32)
        rmse, counts = _run(a, b)
        want, want_counts = R.distance(a, b, [0] * 3, [F] * 3)
        assert np.all(np.abs(rmse - want) <= 1e-9 * want) and np.array_equal(counts, want_counts)
        assert np.all(np.abs(rmse - abs(cents)) < 1e-3)  # (the float32 rounding of b: 2^-24 relative is 1e-4 cents)
        assert counts[:, 0].tolist() == [F] * 3 and not counts[:, 1:3].any()
    # e = 1200 log2(b / a): the same track against itself is exactly 0
    assert _run(a, a)[0].tolist() == [0.0] * 3


def test_planted_flips_and_an_octave_error_give_exact_counts():
    a = _tracks(1)
    b = a.copy()
    b[0, [3, 70, 149]] = 0.0           # voiced -> unvoiced
    a[0, [10, 11]] = 0.0               # unvoiced -> voiced
    a[0, 20] = b[0, 20] = 0.0          # unvoiced in both: neither
    b[0, 100] = 2.0 * a[0, 100]        # an octave: |a / b - 1| = 0.5
    b[1, 5] = a[1, 5] / 1.25           # |a / b - 1| = 0.25 > 0.2
    b[1, 6] = a[1, 6] / 1.15           # 0.15: not gross
    rmse, counts = _run(a, b)
    want, want_counts = R.distance(a, b, [0] * 3, [F] * 3)
    assert np.array_equal(counts, want_counts)
    assert counts.tolist() == [[F - 6, 5, 1, F], [F, 0, 1, F], [F, 0, 0, F]]
    assert np.all(np.abs(rmse - want) <= 1e-9 * want) and rmse[2] == 0.0
    assert abs(rmse[0] - math.sqrt(1200.0 ** 2 / (F - 6))) <= 1e-9 * rmse[0]
    # another ratio moves the gross count alone
    assert _run(a, b, gross_ratio=0.1)[1][:, 2].tolist() == [1, 2, 0]
    assert _run(a, b, gross_ratio=0.6)[1][:, 2].tolist() == [0, 0, 0]


def test_frames_outside_the_span_are_not_read_and_an_empty_span_gives_zeros():
    a, b = _tracks(2), _tracks(3)
    first, count = [10, 0, 149], [100, 0, 1]
    want, want_counts = R.distance(a, b, first, count)
    pa, pb = a.copy(), b.copy()
    for s, (f0, n) in enumerate(zip(first, count)):
        pa[s, :f0] = pb[s, :f0] = np.nan
        pa[s, f0 + n:] = pb[s, f0 + n:] = np.nan
    rmse, counts = _run(pa, pb, first, count)
    assert np.all(np.abs(rmse - want) <= 1e-9 * want) and np.array_equal(counts, want_counts)
    assert rmse[1] == 0.0 and counts[1].tolist() == [0, 0, 0, 0] and counts[:, 3].tolist() == count
    # a NaN inside a span is an unvoiced frame, not a NaN result
    pa[0, 50] = np.nan
    rmse, counts = _run(pa, pb, first, count)
    assert np.all(np.isfinite(rmse)) and counts[0].tolist() == [99, 1, want_counts[0, 2] - (
        abs(float(a[0, 50]) / float(b[0, 50]) - 1.0) > 0.2), 100]


def test_two_calls_and_rows_alone_give_the_same_bits():
    a, b = _tracks(4), _tracks(5)
    b[:, ::7] = 0.0
    x, y = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    one, two = ops.pitch_distance(x, y), ops.pitch_distance(x, y)
    for k in one:
        assert torch.equal(one[k], two[k]), k
    for s in range(3):
        alone = ops.pitch_distance(x[s:s + 1], y[s:s + 1])
        for k in one:
            assert torch.equal(alone[k][0], one[k][s]), (k, s)


def test_refusals():
    x = torch.zeros(2, 9, device=DEV)
    for bad in (dict(first=[0, 5], count=[9, 5]), dict(first=[-1, 0]), dict(first=[0]), dict(count=[10, 1])):
        with pytest.raises(ValueError):
            ops.pitch_distance(x, x, **bad)
    for bad in (0.0, -0.2, float("inf"), float("nan"), True):
        with pytest.raises(ValueError, match="gross_ratio"):
            ops.pitch_distance(x, x, gross_ratio=bad)
    with pytest.raises(ValueError, match="period_b"):
        ops.pitch_distance(x, x[:, :8])
    with pytest.raises(ValueError, match="period_a"):
        ops.pitch_distance(x.double(), x.double())
