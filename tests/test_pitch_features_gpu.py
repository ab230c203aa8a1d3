"""GPU: mvn_pitch_features on planted period tracks against the float64 restatement
(tests/pitch_features_reference): one and two frames, rows without a voiced frame beside fully voiced ones, leading and
trailing gaps, gaps that end at a wave's and at a chunk's boundary +- 1, a gap longer than a chunk (the carry alone makes
it right), NaN and negative periods, a shift per sequence.

Bounds (pitch_features_reference.tolerance): the voiced flag exact; a voiced frame's -- and a held frame's -- log-F0
within 1 fp32 ulp of the reference, which follows from "formed in double, rounded once"; an interpolated frame within
LERP_ULPS = 6 ulps of max(|lf[p]|, |lf[n]|), derived there from the roundings of the lerp on neighbours 1 ulp off.
Measured on an MI355X over the cases here: the largest deviation of an interpolated frame was 1.342 of those ulps (1205
frames), of a voiced or held frame 0.500 ulp."""
import functools

import numpy as np
import pytest
import torch

import pitch_features_reference as R
from helpers import DEV
from movenet_amd import ops

pytestmark = pytest.mark.gpu
CASES = sorted(R.cases())


@functools.lru_cache(maxsize=None)
def _case(name):
    period = R.cases()[name]
    ref = R.features(period)
    return period, ref, R.tolerance(period, ref)


def _run(period, **kw):
    return ops.pitch_features(torch.from_numpy(np.ascontiguousarray(period)).to(DEV), R.RATE, R.F_REF, **kw)


@pytest.mark.parametrize("name", CASES)
def test_matches_the_float64_reference(name):
    period, ref, tol = _case(name)
    B, F = period.shape
    got = _run(period).cpu().numpy()
    assert got.shape == (B, 2, F) and got.dtype == np.float32
    assert np.array_equal(got[:, 1], ref[:, 1].astype(np.float32))           # exactly 0.0 / 1.0
    assert not np.isnan(got).any()
    err = np.abs(got[:, 0].astype(np.float64) - ref[:, 0])
    lerp = R.interpolated(period)
    with np.errstate(divide="ignore", invalid="ignore"):
        ulps = np.where(tol > 0, err / np.where(lerp, tol / R.LERP_ULPS, tol), 0.0)
    print(f"{name}: worst voiced/held frame {ulps[~lerp].max(initial=0.0):.3f} ulp, worst interpolated frame "
          f"{ulps[lerp].max(initial=0.0):.3f} ulps of max(|lf[p]|, |lf[n]|) over {int(lerp.sum())} frames")
    assert (err <= tol).all(), (name, np.argwhere(err > tol)[:5])
    dead = ~R.voiced_of(period).any(axis=1)
    assert np.array_equal(got[dead, 0], np.zeros((int(dead.sum()), F), dtype=np.float32))   # no voiced frame: zeros


@pytest.mark.parametrize("name", ["two_frames", "edges_and_wave_boundary", "long_gap"])
def test_writes_the_last_two_channels_of_a_wider_tensor_and_nothing_else(name):
    period = _case(name)[0]
    B, F = period.shape
    M, ld = 5, F + 3
    plain = _run(period)
    wide = torch.full((B, M + 2, ld), float("nan"), device=DEV)
    back = _run(period, out=wide[:, :, :F])
    assert back.data_ptr() == wide.data_ptr()
    assert torch.equal(wide[:, M:, :F], plain) and not torch.isnan(wide[:, M:, :F]).any()
    assert torch.isnan(wide[:, :M]).all() and torch.isnan(wide[:, M:, F:]).all()


def test_same_bits_on_every_call_and_at_every_batch_position():
    period = np.concatenate([_case("chunk_boundary")[0], _case("long_gap")[0], _case("nan_and_negative")[0]])
    B = period.shape[0]
    first = _run(period)
    assert torch.equal(first, _run(period))
    order = np.roll(np.arange(B), 5)[::-1].copy()
    moved = _run(period[order])
    assert torch.equal(moved, first[torch.from_numpy(order).to(DEV)])
    alone = _run(period[7:8])                      # a row on its own: another grid, the same bits
    assert torch.equal(alone[0], first[7])


def test_shift_is_one_float_add_per_sequence():
    period = _case("edges_and_wave_boundary")[0]
    B = period.shape[0]
    base = _run(period).cpu().numpy()
    shift = np.linspace(-1.0, 1.0, B).astype(np.float32)
    for given in (shift, torch.from_numpy(shift), torch.from_numpy(shift).to(DEV), shift.tolist()):
        got = _run(period, shift=given).cpu().numpy()
        assert np.array_equal(got[:, 0], base[:, 0] + shift[:, None])          # (float32 + float32, one rounding)
        assert np.array_equal(got[:, 1], base[:, 1])
    one = _run(period, shift=1.0).cpu().numpy()
    assert np.array_equal(one[:, 0], base[:, 0] + np.float32(1.0)) and np.array_equal(one[:, 1], base[:, 1])
    for zero in (None, 0, 0.0, [0.0] * B):
        assert np.array_equal(_run(period, shift=zero).cpu().numpy(), base)
    dead = _run(np.zeros((2, 40), dtype=np.float32), shift=[0.25, -2.0]).cpu().numpy()
    assert np.array_equal(dead[:, 0], np.repeat(np.float32([[0.25], [-2.0]]), 40, axis=1)) and not dead[:, 1].any()


def test_refusals_before_any_launch():
    period = torch.zeros(2, 9, device=DEV)
    for bad in (dict(rate=0.0), dict(rate=float("nan")), dict(f_ref=-1.0), dict(f_ref=float("inf")), dict(rate=1e300)):
        with pytest.raises(ValueError, match="finite number above 0"):
            ops.pitch_features(period, **{"rate": 8000.0, "f_ref": 100.0, **bad})
    for bad in (torch.zeros(2, 9, device=DEV, dtype=torch.float64), torch.zeros(9, device=DEV),
                torch.zeros(2, 0, device=DEV)):
        with pytest.raises(ValueError, match="period"):
            ops.pitch_features(bad, 8000.0, 100.0)
    for out in (torch.zeros(2, 1, 9, device=DEV), torch.zeros(2, 3, 8, device=DEV), torch.zeros(3, 3, 9, device=DEV),
                torch.zeros(2, 3, 9, device=DEV, dtype=torch.float64), torch.zeros(2, 3, 18, device=DEV)[:, :, ::2],
                torch.zeros(2, 9, 3, device=DEV).transpose(1, 2), torch.zeros(3, 9, device=DEV).expand(2, 3, 9)):
        with pytest.raises(ValueError, match="out must be"):
            ops.pitch_features(period, 8000.0, 100.0, out=out)
    with pytest.raises(ValueError, match="shift"):
        ops.pitch_features(period, 8000.0, 100.0, shift=[1.0, 2.0, 3.0])
