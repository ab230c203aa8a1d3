"""GPU: ``ops.feature_distance`` (mvn_feature_distance) against the float64 numpy restatement
(tests/spectral_reference.py) on the same float32 inputs.

Tolerance, derived: every sum is over n non-negative doubles, so any summation order agrees with any other to
(n - 1) 2^-53 relative; with n <= M F = 24 000 in these shapes that is at most 2.7e-12, and ``RTOL = 1e-11`` leaves
room for the square root and the divisions.  ``per_frame`` is float32: ``2^-23`` relative."""
import math

import numpy as np
import pytest
import torch

import spectral_reference as R
from helpers import DEV
from movenet_amd import ops

pytestmark = pytest.mark.gpu
RTOL, RTOL_F32 = 1e-11, 2.0 ** -23
DB = 10.0 / math.log(10.0)
BLOCK = 256   # frames per workgroup of mvn_feature_distance (csrc/metrics.hip: kFrames)


def _inputs(B, M, F, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(B, M, F)) * 3.0).astype(np.float32), (rng.normal(size=(B, M, F)) * 3.0).astype(np.float32)


def _run(a, b, first=None, count=None, per_frame=True):
    out = ops.feature_distance(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), first, count,
                               per_frame=per_frame)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(got, a, b, first, count):
    lsd, l1, pf = R.feature_distance(a, b, first, count)
    print("lsd_db", got["lsd_db"], "max rel err", np.max(np.abs(got["lsd_db"] - lsd) / np.maximum(lsd, 1e-300)),
          "l1 max rel err", np.max(np.abs(got["l1"] - l1) / np.maximum(l1, 1e-300)))
    assert got["lsd_db"].dtype == np.float64 and got["l1"].dtype == np.float64 and got["frames"].dtype == np.int32
    assert np.array_equal(got["frames"], np.asarray(count if count is not None else [a.shape[2]] * a.shape[0]))
    assert np.all(np.isfinite(got["lsd_db"])) and np.all(np.isfinite(got["l1"]))
    assert np.allclose(got["lsd_db"], lsd, rtol=RTOL, atol=0)
    assert np.allclose(got["l1"], l1, rtol=RTOL, atol=0)
    if "per_frame" in got:
        assert got["per_frame"].dtype == np.float32 and got["per_frame"].shape == pf.shape
        assert np.allclose(got["per_frame"], pf, rtol=RTOL_F32, atol=0)
        assert np.array_equal(got["per_frame"] == 0, pf == 0)   # exactly 0 outside the span (and only there)


def test_smallest_shape_with_an_empty_span_between_two_full_ones():
    a, b = _inputs(3, 5, 1, 1)
    first, count = [0, 0, 0], [1, 0, 1]
    got = _run(a, b, first, count)
    _check(got, a, b, first, count)
    assert got["lsd_db"][1] == 0.0 and got["l1"][1] == 0.0 and got["frames"][1] == 0
    assert got["lsd_db"][0] > 0 and got["l1"][2] > 0


@pytest.fixture(scope="module")
def two_rows():
    a, b = _inputs(2, 80, 300, 2)
    first, count = [3, 299], [290, 1]
    return a, b, first, count, _run(a, b, first, count)


def test_frames_past_one_workgroup_and_a_single_last_frame(two_rows):
    a, b, first, count, got = two_rows
    _check(got, a, b, first, count)


def test_default_span_is_every_frame_and_spans_come_as_arrays_or_tensors(two_rows):
    a, b, first, count, got = two_rows
    _check(_run(a, b, per_frame=False), a, b, None, None)
    for conv in (np.asarray, torch.tensor, lambda v: torch.tensor(v, device=DEV)):
        again = _run(a, b, conv(first), conv(count))
        assert all(np.array_equal(again[k], got[k]) for k in got)


def test_a_sequence_over_several_workgroups():
    F = 2 * BLOCK + 3
    a, b = _inputs(1, 64, F, 3)
    for first, count in (([0], [F]), ([BLOCK - 1], [BLOCK + 2]), ([2 * BLOCK], [3]), ([5], [7])):
        _check(_run(a, b, first, count), a, b, first, count)


def test_planted_offset_is_exact():
    rng = np.random.default_rng(4)
    b = (rng.integers(-8192, 8193, size=(2, 80, 300)) / 1024.0).astype(np.float32)   # multiples of 2^-10 in [-8, 8]
    a = b + np.float32(0.25)
    assert np.array_equal(a.astype(np.float64) - b.astype(np.float64), np.full(b.shape, 0.25))
    got = _run(a, b, [3, 299], [290, 1])
    assert np.array_equal(got["l1"], [0.25, 0.25])
    assert np.allclose(got["lsd_db"], 0.25 * DB, rtol=RTOL, atol=0)
    assert np.allclose(got["per_frame"][0, 3:293], np.float32(0.25 * DB), rtol=RTOL_F32, atol=0)


def test_nothing_outside_the_span_is_read_and_every_output_is_written():
    a, b = _inputs(2, 80, 300, 5)
    first, count = [3, 299], [290, 1]
    poison = (np.nan, np.inf, -np.inf)
    for s, (f0, n) in enumerate(zip(first, count)):
        for x in (a, b):
            outside = np.ones(300, bool)
            outside[f0:f0 + n] = False
            x[s][:, outside] = np.resize(poison, (80, int(outside.sum())))
    got = _run(a, b, first, count)
    _check(got, a, b, first, count)
    assert not got["per_frame"][0, :3].any() and not got["per_frame"][0, 293:].any() and not got["per_frame"][1, :299].any()
    # the C entry itself, into buffers (the scratch included) that hold NaN: everything read back was written
    from movenet_amd import _native as N
    from movenet_amd.generation import _stream_ptr
    lib = N.lib()
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    span = torch.tensor(first + count, dtype=torch.int32, device=DEV)
    n = lib.mvn_feature_distance_scratch_floats(2, 300)
    assert n == 4 * 2 * 2
    lsd, l1, scratch = (torch.full((k,), float("nan"), dtype=torch.float64, device=DEV) for k in (2, 2, n // 2))
    pf = torch.full((2, 300), float("nan"), dtype=torch.float32, device=DEV)
    with torch.cuda.device(ta.device):
        N.check(lib.mvn_feature_distance(ta.data_ptr(), tb.data_ptr(), 2, 80, 300, span.data_ptr(), span[2:].data_ptr(),
                                         lsd.data_ptr(), l1.data_ptr(), pf.data_ptr(), scratch.data_ptr(), n,
                                         _stream_ptr(ta.device)), "mvn_feature_distance")
    assert lsd.cpu().numpy().tobytes() == got["lsd_db"].tobytes() and l1.cpu().numpy().tobytes() == got["l1"].tobytes()
    assert pf.cpu().numpy().tobytes() == got["per_frame"].tobytes()
    assert bool(torch.isfinite(scratch).all())


def test_the_same_bits_on_every_call_and_in_every_batch(two_rows):
    a, b, first, count, got = two_rows
    again = _run(a, b, first, count)
    assert all(again[k].tobytes() == got[k].tobytes() for k in got)
    alone = _run(a[1:], b[1:], first[1:], count[1:])
    assert all(alone[k].tobytes() == got[k][1:].tobytes() for k in got)
    alone0 = _run(a[:1], b[:1], first[:1], count[:1])
    assert all(alone0[k].tobytes() == got[k][:1].tobytes() for k in got)


def test_refusals_launch_nothing(monkeypatch):
    a = torch.zeros(2, 5, 300, device=DEV)
    torch.cuda.synchronize()
    from movenet_amd import _native as N
    real = N.lib()

    class Refuse:
        def __getattr__(self, name):
            if name == "mvn_feature_distance":
                pytest.fail("mvn_feature_distance was called")
            return getattr(real, name)
    monkeypatch.setattr(N, "lib", lambda: Refuse())
    for first, count in (([0, 299], [300, 2]), ([0, -1], [300, 1]), ([0, 0], [300, -1]), ([0], [300]),
                         ([0, 0.5], [300, 1]), ([0, 301], [300, 0])):
        with pytest.raises(ValueError):
            ops.feature_distance(a, a, first, count)
    with pytest.raises(ValueError, match="float32"):
        ops.feature_distance(a, torch.zeros(2, 5, 299, device=DEV))
    with pytest.raises(ValueError, match="float32"):
        ops.feature_distance(a, torch.zeros(2, 6, 300, device=DEV))
    with pytest.raises(ValueError, match="float32"):
        ops.feature_distance(a.double(), a.double())
    with pytest.raises(ValueError, match="float32"):
        ops.feature_distance(a, a.double())
    with pytest.raises(ValueError, match="float32"):
        ops.feature_distance(a[0], a[0])
    # a non-contiguous view is taken as its contiguous copy
    monkeypatch.undo()
    t = torch.randn(2, 300, 5, device=DEV).transpose(1, 2)
    u = torch.randn(2, 5, 300, device=DEV)
    assert not t.is_contiguous()
    want = ops.feature_distance(t.contiguous(), u)
    got = ops.feature_distance(t, u)
    assert torch.equal(got["lsd_db"], want["lsd_db"]) and torch.equal(got["l1"], want["l1"])
