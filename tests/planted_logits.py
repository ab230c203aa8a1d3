"""Planted logits for the sampling tests: a network whose head returns a KNOWN vector at every step, and the table of
(design, rule, T, top_k, top_p) rows that tests/test_planted_logits_host.py proves decidable and
tests/test_sampling_edges_gpu.py runs on every generator kernel.  Numpy / torch only, no device.

The device.  With dense_conv.conv2.weight = 0 and dense_conv.conv2.bias = the planted vector, every step's logits are
exactly the bias whatever the history (the kernels add b2 to a sum of exact zeros), while every layer, queue and
hand-off of the network still runs.  The planted vector is a few TIE GROUPS over a floor: equal logits give bit-equal
fp32 weights under either sampling rule, so the kept set that include/movenet_hip.h prescribes ("exact ties at the
threshold are all kept") is a union of whole groups, decided by the gaps between the groups and not by rounding.

Designs (``design(name, Q)``), all generated from seeds:
  five      3.0 x 3 classes, 2.0 x 5, 0.5 x 8, -1.0 x 16, floor -6.0; the classes permuted by default_rng(1000 + Q)
  wide      the same classes at ten times the logits (30, 20, 5, -10, -60): at T = 1e4 its groups are still 1e-3
            apart relatively, where five's 1e-4 is below the 2^-10 the host file asks of a threshold
  straddle  the maximum 3.0 tied across a 64-class boundary AND held by the last class: classes 63, 64 and Q - 1
            (Q = 64: 31, 32 and 63); 1.5 at classes 0, 1 and either side of the pair; floor -2.0.  Not permuted: the
            point is where the members sit (GENERIC / STREAM: lane 63 of one trip and lane 0 of the next; the
            pipelined heads: the last lane of one DPP row and the first of the next)
  untied / tied   Q = 2 only: {0, -1} and {0, 0}
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np
import torch

import truncation_reference as TR

Row = namedtuple("Row", "design rule T k p")  # top_k = 0 / top_p = 1.0: off
GAP_MIN = 2.0 ** -10  # (d) of the host file: far above TR.TIE_EPS = 2^-18, no hardware exp reorders such groups
FIVE_GROUPS = ((3.0, 3), (2.0, 5), (0.5, 8), (-1.0, 16))
FIVE_FLOOR = -6.0
TEMPERATURES = (0.02, 0.25, 1.0, 4.0, 1e4)


@functools.lru_cache(maxsize=None)
def _design(name: str, Q: int) -> np.ndarray:
    if Q == 2:
        return np.array({"untied": [0.0, -1.0], "tied": [0.0, 0.0]}[name], dtype=np.float32)
    if name in ("five", "wide"):
        assert Q >= 64
        out = np.full(Q, FIVE_FLOOR, dtype=np.float32)
        perm, at = np.random.default_rng(1000 + Q).permutation(Q), 0
        for value, count in FIVE_GROUPS:
            out[perm[at:at + count]] = value
            at += count
        return out * np.float32(10.0 if name == "wide" else 1.0)
    if name == "straddle":
        assert Q >= 64
        a = 63 if Q > 64 else 31
        out = np.full(Q, -2.0, dtype=np.float32)
        out[[0, 1, a - 1, a + 2]] = 1.5
        out[[a, a + 1, Q - 1]] = 3.0
        return out
    raise KeyError(name)


def design(name: str, Q: int) -> np.ndarray:
    """The planted fp32 logits (Q,) of a design; a fresh copy."""
    return _design(name, Q).copy()


def groups(logits) -> list:
    """The tie groups of a planted vector: boolean masks, by descending logit."""
    logits = np.asarray(logits)
    return [logits == v for v in np.unique(logits)[::-1]]


def plant(state_dict, logits):
    """A copy of ``state_dict`` whose head returns ``logits`` at every step: conv2.weight = 0, conv2.bias = logits."""
    sd = dict(state_dict)
    w, b = sd["dense_conv.conv2.weight"], sd["dense_conv.conv2.bias"]
    planted = torch.as_tensor(np.asarray(logits, dtype=np.float32))
    assert planted.shape == b.shape, (planted.shape, b.shape)
    sd["dense_conv.conv2.weight"] = torch.zeros_like(w)
    sd["dense_conv.conv2.bias"] = planted.to(b.device)
    return sd


# ---- the weights of a row: float64, and as an fp32 kernel forms them -------------------------------------------
def weights64(logits, rule: str, T: float) -> np.ndarray:
    return (TR.model_weights if rule == "model" else TR.reference_weights)(logits, T)


def weights32(logits, rule: str, T: float) -> np.ndarray:
    """numpy float32 exp of the float32 argument, every intermediate in float32."""
    l, t = np.asarray(logits, dtype=np.float32), np.float32(T)
    if rule == "model":
        w = np.exp((l - l.max()) / t)
    else:
        e = np.exp(l - l.max())
        x = e / e.sum(dtype=np.float32) / t
        w = np.exp(x - x.max())
    assert w.dtype == np.float32
    return w


def defects(logits, rule: str, T: float, k: int, p: float) -> list:
    """Why a row is NOT decidable; empty for a row that may stand in the table.  (a) - (d) of the host file."""
    logits = np.asarray(logits, dtype=np.float32)
    out = []
    w = weights64(logits, rule, T)
    kept = TR.kept_set(w, k, p)
    if any(kept[g].any() != kept[g].all() for g in groups(logits)):
        out.append("(a) the float64 kept set splits a tie group")
    if p < 1.0:
        lo, hi = TR.kept_set(w, k, p * (1.0 - TR.SUM_EPS)), TR.kept_set(w, k, min(1.0, p * (1.0 + TR.SUM_EPS)))
        if not (np.array_equal(lo, kept) and np.array_equal(hi, kept)):
            out.append("(b) the kept set changes between p (1 - SUM_EPS) and p (1 + SUM_EPS)")
    w32 = weights32(logits, rule, T).astype(np.float64)
    pos = w32 > 0
    if not np.array_equal(TR.kept_set(w32, k, p)[pos], kept[pos]):
        out.append("(c) the fp32 weights give another kept set on classes of positive fp32 weight")
    if not (kept & pos).any():
        out.append("(c) no kept class has a positive fp32 weight")
    elif (~kept & pos).any():
        thr, below = w32[kept & pos].min(), w32[~kept & pos].max()
        if not (thr - below) / thr >= GAP_MIN:
            out.append(f"(d) the threshold group leads the next by {(thr - below) / thr:.3g} < 2^-10, relatively")
    return out


# ---- the table -------------------------------------------------------------------------------------------------
# (variant, shape, Q, B, n_new).  G: 2 x 2 layers, C = K = 16; S64: 4 x 1 layers, C = K = 64; S128: 5 x 2 layers,
# C = K = 128 -- the smallest shapes each kernel takes.  FOLD at Q = 64 runs the 256-wide head with 192 padded classes.
SHAPES = {"G": (2, 2, 16), "S64": (4, 1, 64), "S128": (5, 2, 128)}
RUNS = ([("GENERIC", "G", Q, 16, 500 if Q < 257 else 300) for Q in (2, 100, 200, 257, 1000, 1024)] +
        [(v, "S64", Q, 16, 700) for Q in (128, 256) for v in ("STREAM", "PIPE", "FOLD")] +
        [("FOLD", "S64", 64, 16, 700), ("PIPE_F16", "S128", 256, 8, 300)])


def shape_config(shape: str, Q: int) -> dict:
    layer_size, stack_size, C = SHAPES[shape]
    return dict(layer_size=layer_size, stack_size=stack_size, input_channels=Q, residual_channels=C, skip_channels=C)


def pool(Q: int) -> list:
    """The knob rows at T = 1 and T = 0.25, both designs: thresholds inside a tie group (five: k = 1, 2, 4, 9, Q - 1;
    straddle: k = 1, 2, 4, 8, 9, Q - 1) and on its edge (five: k = 3, 8; straddle: k = 3)."""
    out = []
    for T in (1.0, 0.25):
        for d in ("five", "straddle"):
            out += [Row(d, "model", T, k, 1.0) for k in (1, 2, 3, 4, 8, 9, Q - 1)]
            out += [Row(d, "model", T, 0, p) for p in (1e-6, 0.3, 0.6, 0.9, 0.999)]
            out.append(Row(d, "model", T, 9, 0.5))
    return out


def always(Q: int) -> list:
    """The rows every kernel and shape runs: every temperature without truncation, one top-k and one top-p row at
    each extreme temperature, and the reference rule's rows."""
    return ([Row("five", "model", T, 0, 1.0) for T in TEMPERATURES] +
            [Row("five", "model", 0.02, 4, 1.0), Row("five", "model", 0.02, 0, 0.9),
             # T = 1e4: every weight within 1 % of 1.  k = 4 ends inside the second group; p = 5.5 / Q asks for 5.5 of
             # the ~Q total: more than the top group's 3, less than the first two groups' 8
             Row("wide", "model", 1e4, 4, 1.0), Row("wide", "model", 1e4, 0, round(5.5 / Q, 4))] +
            [Row("five", "reference", 1.0, k, 1.0) for k in (3, 4, 8)] +
            [Row("straddle", "reference", 1.0, 1, 1.0), Row("five", "reference", 1.0, 0, 1e-6),
             Row("five", "reference", 1.0, 0, 0.3)])


TWO_CLASS_ROWS = ([Row("untied", "model", T, 0, 1.0) for T in TEMPERATURES] +
                  [Row("tied", "model", 1.0, 0, 1.0), Row("tied", "model", 1.0, 1, 1.0),
                   Row("untied", "model", 1.0, 1, 1.0), Row("untied", "model", 0.25, 1, 1.0),
                   Row("untied", "model", 1.0, 0, 1e-6), Row("untied", "model", 1.0, 0, 0.6),
                   Row("untied", "model", 1.0, 0, 0.9), Row("tied", "model", 1.0, 0, 0.6),
                   Row("tied", "model", 0.25, 0, 1e-6), Row("untied", "model", 0.02, 1, 1.0),
                   Row("untied", "model", 0.02, 0, 0.9), Row("untied", "model", 1e4, 0, 0.3),
                   Row("untied", "model", 1e4, 0, 0.9),
                   Row("tied", "reference", 1.0, 1, 1.0), Row("untied", "reference", 1.0, 1, 1.0),
                   Row("untied", "reference", 1.0, 0, 0.5), Row("untied", "reference", 1.0, 0, 0.9)])

# Rows the host file's conditions reject: deleted here, with the reason, not skipped at run time.
DELETED = {
    # w = {1, exp(-1e-4)}: p S = 0.6 keeps class 0 alone, 1e-4 above the class it drops -- (d)
    (2, Row("untied", "model", 1e4, 0, 0.3)): "(d) the threshold leads the dropped class by 1e-4 < 2^-10",
}

POOL_SHARE = 8  # pool rows per run: the 13 runs with Q >= 64 go round the 52-row pool twice


def rows_of(run_index: int) -> list:
    """The rows of RUNS[run_index]."""
    variant, shape, Q, B, n_new = RUNS[run_index]
    if Q == 2:
        rows = list(TWO_CLASS_ROWS)
    else:
        pl = pool(Q)
        at = sum(1 for r in RUNS[:run_index] if r[2] != 2) * POOL_SHARE
        rows = always(Q) + [pl[(at + j) % len(pl)] for j in range(POOL_SHARE)]
    return [r for r in rows if (Q, r) not in DELETED]


def table() -> list:
    """Every (run, row) of the two test files: [(variant, shape, Q, B, n_new, Row)]."""
    return [run + (row,) for i, run in enumerate(RUNS) for row in rows_of(i)]


# The row of the history-independence and conditioning checks of the GPU file (five at T = 1: k = 9 ends inside the
# third group, 16 classes; p = 0.9 of their mass needs more than the first two groups' 88 %: all 16 stay), and the
# indices into RUNS of the runs that make them: one per kernel / one each for GENERIC, STREAM and FOLD.
HISTORY_ROW = Row("five", "model", 1.0, 9, 0.9)
HISTORY_RUNS = (3, 7, 9, 12, 13)   # GENERIC Q = 257, PIPE 128, STREAM 256, FOLD 64, PIPE_F16 256
CONDITIONED_RUNS = (2, 6, 11)      # GENERIC Q = 200, STREAM 128, FOLD 256


def emulate_draws(logits, row: Row, uniform, mutation: int = 0) -> np.ndarray:
    """The picks of a sampled step as an fp32 kernel forms them, in numpy: the weights of ``weights32``, the exact
    thresholds of the radix select (top-k: the k-th largest bit pattern; top-p: the largest weight value whose head
    reaches the fp32 product p * S in an fp32 sum), GENERIC's serial running sum, in double, against uniform * total.
    ``mutation`` 1 keeps `> theta` where the header says `>=`; 2 counts `> top_k` where it says `>=` (the select then
    ends on the (k + 1)-th largest weight).  The host file shows the GPU file's checks pass the one and catch the others."""
    w = weights32(logits, row.rule, row.T).copy()
    bits, Q, zero = w.view(np.uint32), w.size, np.float32(0)
    theta = np.uint32(0)
    if 0 < row.k < Q:
        theta = np.sort(bits)[::-1][row.k if mutation == 2 else row.k - 1]
    if row.p < 1.0:
        def mass_from(lo):
            return np.cumsum(np.where(bits >= lo, w, zero), dtype=np.float32)[-1]
        need = np.float32(row.p) * mass_from(theta)
        tp = next((v for v in np.unique(bits)[::-1] if v > 0 and mass_from(max(v, theta)) >= need), np.uint32(0))
        theta = max(tp, theta)
    keep = bits > theta if mutation == 1 else bits >= theta
    fallback = np.nonzero(keep)[0].max() if keep.any() else Q - 1
    cdf = np.cumsum(np.where(keep, w, zero), dtype=np.float64)
    target = np.asarray(uniform, dtype=np.float32).astype(np.float64) * cdf[-1]
    at = np.searchsorted(cdf, target, side="right")
    return np.where(at < Q, at, fallback).astype(np.int32)


def row_id(row: Row) -> str:
    return f"{row.design}-{row.rule}-T{row.T:g}-k{row.k}-p{row.p:g}"
