"""GPU: the de-emphasising PCM conversion (mvn_pcm16_deemph_chunk, ops.pcm16_chunk(deemphasis=a, state=...)) against the
sequential float64 loop of tests/emphasis_reference.py -- EXACTLY: the PCM, and the carried state bit for bit.  The
recurrence is defined sequentially, so the same clip in chunks of any size gives the same bits, from output views on odd
and on even int16 addresses; views of a larger sample tensor work; nothing outside the written columns is touched; the
refusals come before any launch."""
import ctypes
import math

import numpy as np
import pytest
import torch

import emphasis_reference as R
from movenet_amd import _native as N
from movenet_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Q, T, A = 256, 2500, 0.97
SENTINEL = -32768   # never a PCM value: the conversion clips to [-32767, 32767]
BATCHES = [3, 300]


def _classes(B, seed=5):
    """(B, T) random classes, a share of them outside [0, Q) on either side"""
    g = torch.Generator().manual_seed(seed + B)
    return torch.randint(-6, Q + 6, (B, T), generator=g, dtype=torch.int32)


_CASES: dict = {}


def _case(B):
    """classes on the device, and the reference's PCM and final state for the whole clip -- computed once per B"""
    if B not in _CASES:
        cls = _classes(B).to(DEV)
        x = ops.mu_law_decode(cls.clamp(0, Q - 1), Q).cpu().numpy()
        assert x.dtype == np.float32
        pcm, state = R.deemph_pcm16(x, A)
        pcm.setflags(write=False)
        state.setflags(write=False)
        _CASES[B] = (cls, pcm, state)
    return _CASES[B]


def _bits(t):
    return t.cpu().numpy().view(np.int64)


@pytest.mark.parametrize("B", BATCHES)
def test_whole_clip_is_the_sequential_reference_to_the_bit(B):
    cls, want, want_state = _case(B)
    state = torch.zeros(B, dtype=torch.float64, device=DEV)
    got = ops.pcm16_chunk(cls, 0, T, Q, deemphasis=A, state=state).cpu().numpy()
    assert got.dtype == np.int16 and got.shape == (B, T)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.array_equal(_bits(state), want_state.view(np.int64))
    assert np.array_equal(ops.deemphasis_pcm16(cls, A, Q).cpu().numpy(), want)
    # the filter does something: the plain conversion of these classes is another signal
    assert not np.array_equal(ops.pcm16_chunk(cls, 0, T, Q).cpu().numpy(), want)
    assert np.array_equal(ops.deemphasis_pcm16(cls, 0.0, Q).cpu().numpy(), ops.pcm16_chunk(cls, 0, T, Q).cpu().numpy())


@pytest.mark.parametrize("chunk", [1, 7, 64, 65, 1000])
@pytest.mark.parametrize("B", BATCHES)
def test_chunks_of_any_size_give_the_bits_of_the_whole_clip(B, chunk):
    cls, want, want_state = _case(B)
    state = torch.zeros(B, dtype=torch.float64, device=DEV)
    band, stride = 8, chunk + 3   # (an odd gap between rows where chunk is even: every other row starts on an odd int16)
    bufs = [torch.full((2 * band + B * stride + 1,), SENTINEL, dtype=torch.int16, device=DEV) for _ in range(2)]
    views = [buf[band + off:band + off + B * stride].view(B, stride) for off, buf in enumerate(bufs)]
    assert [v.data_ptr() % 4 for v in views] == [0, 2]
    got = torch.empty(B, T, dtype=torch.int16, device=DEV)
    for k, t0 in enumerate(range(0, T, chunk)):
        n = min(chunk, T - t0)
        got[:, t0:t0 + n] = ops.pcm16_chunk(cls, t0, n, Q, out=views[k % 2], deemphasis=A, state=state)
    got = got.cpu().numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.array_equal(_bits(state), want_state.view(np.int64))
    for off, buf in enumerate(bufs):   # nothing but the rows' first `chunk` columns was ever written
        flat = buf.cpu().numpy()
        rows = flat[band + off:band + off + B * stride].reshape(B, stride)
        assert np.all(flat[:band + off] == SENTINEL) and np.all(flat[band + off + B * stride:] == SENTINEL)
        assert np.all(rows[:, chunk:] == SENTINEL)


def test_views_of_a_larger_sample_tensor_and_a_poison_band():
    B = 3
    cls, want, want_state = _case(B)
    big = torch.full((B + 4, T + 100), Q // 2, dtype=torch.int32, device=DEV)
    big[2:2 + B, 50:50 + T] = cls
    band = 32
    buf = torch.full((2 * band + B * T,), SENTINEL, dtype=torch.int16, device=DEV)
    out = buf[band:band + B * T].view(B, T)
    state = torch.zeros(B, dtype=torch.float64, device=DEV)
    # a row block that is also a column view, in two calls: the second starts inside the view
    ops.pcm16_chunk(big[2:2 + B, 50:50 + T], 0, 1203, Q, out=out, deemphasis=A, state=state)
    ops.pcm16_chunk(big[2:2 + B, 40:50 + T], 10 + 1203, T - 1203, Q, out=out[:, 1203:], deemphasis=A, state=state)
    flat = buf.cpu().numpy()
    assert np.array_equal(flat[band:band + B * T].reshape(B, T), want)
    assert np.all(flat[:band] == SENTINEL) and np.all(flat[band + B * T:] == SENTINEL)
    assert np.array_equal(_bits(state), want_state.view(np.int64))
    # a state that is a row block of a larger one (what a grouped stream hands each group)
    states = torch.zeros(B + 2, dtype=torch.float64, device=DEV)
    got = ops.pcm16_chunk(cls, 0, T, Q, deemphasis=A, state=states[1:1 + B]).cpu().numpy()
    assert np.array_equal(got, want)
    assert states[0].item() == 0.0 and states[B + 1].item() == 0.0
    assert np.array_equal(_bits(states[1:1 + B]), want_state.view(np.int64))


def test_no_columns_is_a_no_op_that_keeps_the_state():
    cls, _, _ = _case(3)
    state = torch.tensor([0.25, -0.5, 1e-300], dtype=torch.float64, device=DEV)
    before = _bits(state).copy()
    assert tuple(ops.pcm16_chunk(cls, 17, 0, Q, deemphasis=A, state=state).shape) == (3, 0)
    out = torch.full((3, 4), SENTINEL, dtype=torch.int16, device=DEV)
    rc = N.lib().mvn_pcm16_deemph_chunk(cls.data_ptr(), 3, T, 17, 0, Q, A, state.data_ptr(), out.data_ptr(), 4, None)
    assert rc == N.MVN_OK
    torch.cuda.synchronize()
    assert np.array_equal(_bits(state), before) and bool((out == SENTINEL).all())


def test_bad_coefficient_and_bad_state_are_refused_before_any_launch():
    cls, _, _ = _case(3)
    lib = N.lib()
    state = torch.full((4,), 0.125, dtype=torch.float64, device=DEV)
    out = torch.full((3, 8), SENTINEL, dtype=torch.int16, device=DEV)

    def call(coef=A, state_ptr=state.data_ptr(), n=8, classes=Q, t0=0):
        return lib.mvn_pcm16_deemph_chunk(cls.data_ptr(), 3, T, t0, n, classes, coef, state_ptr, out.data_ptr(), 8, None)

    for kw in (dict(coef=1.0), dict(coef=-0.25), dict(coef=math.nan), dict(coef=math.inf), dict(state_ptr=None),
               dict(state_ptr=state.data_ptr() + 4), dict(n=-1), dict(n=9), dict(t0=T - 7), dict(classes=1),
               dict(classes=40000)):
        assert call(**kw) == N.MVN_ERR_BAD_ARG, kw
        assert "mvn_pcm16_deemph_chunk" in N.last_error()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((state == 0.125).all())
    assert call() == N.MVN_OK   # (the same call with nothing wrong goes through)
    torch.cuda.synchronize()
    assert bool((out != SENTINEL).all())
    # ... and ops says so as ValueError, for the coefficient and for a state of the wrong kind
    for bad in (1.0, -0.25, math.nan):
        with pytest.raises(ValueError, match="deemphasis"):
            ops.pcm16_chunk(cls, 0, 8, Q, deemphasis=bad, state=state[:3])
    for bad in (None, state, state[:3].to(torch.float32), torch.zeros(6, dtype=torch.float64, device=DEV)[::2]):
        with pytest.raises(ValueError, match="state"):
            ops.pcm16_chunk(cls, 0, 8, Q, deemphasis=A, state=bad)
    with pytest.raises(RuntimeError, match="state must live on"):   # (the package's error for a host tensor)
        ops.pcm16_chunk(cls, 0, 8, Q, deemphasis=A, state=state[:3].cpu())
