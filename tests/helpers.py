"""Shared helpers for the parity tests (CPU and GPU)."""
from __future__ import annotations

import math

import numpy as np
import torch

from movenet_amd.utils.weights import (
    make_state_dict, one_hot, state_dict_sha256, synthetic_indices,
)
from oracle import wavenet_oracle as O

CFG_KEYS = ("layer_size", "stack_size", "input_channels", "residual_channels", "skip_channels")


def cfg_of(fx) -> dict:
    return dict(zip(CFG_KEYS, (int(v) for v in fx["cfg"])))


def weights_of(fx):
    """Regenerate the fixture's weights from its recipe and check the SHA."""
    kw = {}
    if "gain" in fx.files:
        kw = dict(gain=float(fx["gain"]), head_gain=float(fx["head_gain"]))
    cfg = cfg_of(fx)
    sd = make_state_dict(**cfg, seed=int(fx["weight_seed"]), **kw)
    assert state_dict_sha256(sd) == str(fx["weight_sha"]), "weight recipe drifted from the fixture"
    return cfg, O.Dims(**cfg), sd


def rel_err(a, b) -> float:
    a = torch.as_tensor(np.asarray(a)).double()
    b = torch.as_tensor(np.asarray(b)).double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


# ---- rows past a 32-bit buffer offset (the column loss / softmax kernels, the head strips) ----
# Row q, column t of one (Q, ld) tensor sits at byte offset 4 (q ld + t) from the sequence's base.
OFFSET_LIMIT = 1 << 31


def long_row_lengths(Q: int) -> dict:
    """Row strides at the edge of the 32-bit offset limit of a (Q, ld) fp32 tensor, multiples of 64:
    ``below`` -- every offset fits; ``tail`` -- only the tail columns of the LAST row cross;
    ``past`` -- the rows from about 85 % of Q on start beyond the limit."""
    fit = OFFSET_LIMIT // (4 * Q)                    # first column past the limit in row Q - 1 ... (for ld = fit)
    below = fit // 64 * 64 - 128
    tail = fit // 64 * 64 + 2048
    assert 4 * (Q - 1) * tail < OFFSET_LIMIT < 4 * Q * tail
    past = -(-OFFSET_LIMIT // (4 * Q * 85 // 100)) // 64 * 64 + 64
    return dict(below=below, tail=tail, past=past)


def first_bad_row(Q: int, ld: int) -> int:
    """The first row that starts at or past the limit (Q when none does)."""
    return min(Q, -(-OFFSET_LIMIT // (4 * ld)))


# ---- gradient bounds against a float64 reference ----
GRAD_TOL, GRAD_TOL_MAX = 2e-5, 3e-4


def grad_bound(fp32_deviation: float) -> float:
    """Bound on max |err| / max |ref| of an fp32 gradient against float64: 2e-5 ("fp32 sums in another order"), or,
    where the same reference computed in fp32 on the CPU is itself further than 5e-6 from float64, four times that
    deviation (another summation order may land on the other side) -- never above 3e-4, the loosest gradient bound
    the suite uses against its oracle.  Never derived from the output of the code under test."""
    if fp32_deviation <= 5e-6:
        return GRAD_TOL
    return min(4.0 * fp32_deviation, GRAD_TOL_MAX)


# ---- sentinel bands around the buffers handed to the C ABI (GPU tests) ----
DEV = "cuda:0"
SENTINEL = -1234.5
BAND = 1 << 14                     # elements of sentinel behind (and, with front=True, in front of) every buffer


class _Guard:
    """Buffers carved out of larger allocations, a band of sentinel values behind each and -- ``front=True`` -- in
    front of each (64 KB: the buffer keeps the allocator's alignment)"""

    def __init__(self, front=False):
        self.bands, self.front = [], front

    def new(self, shape, fill=None, name="buffer", dtype=torch.float32):
        n = math.prod(shape)
        lo = BAND if self.front else 0
        raw = torch.empty(lo + n + BAND, dtype=dtype, device=DEV)
        sentinel = SENTINEL if dtype.is_floating_point else int(SENTINEL)
        for band, where in ((raw[:lo], "in front of"), (raw[lo + n:], "past the end of")):
            band.fill_(sentinel)
            self.bands.append((name, tuple(shape), band, sentinel, where))
        out = raw[lo:lo + n].view(shape)
        if fill is not None:
            out.fill_(fill)
        return out

    def put(self, t, name="buffer"):
        out = self.new(tuple(t.shape), name=name, dtype=t.dtype)
        out.copy_(t)
        return out

    def check(self, what):
        torch.cuda.synchronize()
        for name, shape, band, sentinel, where in self.bands:
            bad = int((band != sentinel).sum())
            assert bad == 0, f"{what} wrote {bad} elements {where} {name} {shape}"
