"""GPU: sampled generation on PLANTED logits (tests/planted_logits.py) -- exact ties at the truncation threshold, class
counts that are no multiple of 64, the tuned heads at Q = 128 and 64, and the temperature extremes, on all five
generator kernels and both code forms of the select (truncate_weights / choose_class in csrc/pipe_common.h,
truncate_weights_lds and the block-wide choosers in csrc/generate.hip).

The head's last product is zero and its bias is a vector of tie groups, so every step's logits are known to the bit
and the kept set of include/movenet_hip.h is a union of whole groups; tests/test_planted_logits_host.py proves every row
of the table decidable on the CPU, so NO step of any case is exempted here (share of excluded draws: 0).

On each run (B x n_new teacher-forced draws with the logits returned):
  1. logits_out equals the planted bias bit for bit at every step (PIPE_F16 too: its conv2 accumulates in fp32 and adds
     the fp32 bias last, generate_pipe_h16.hip);
  2. every pick lies in the float64 kept set, ties kept whole;
  3. every draw lies inside the float64 band of its pick on the truncated CDF within eps = 4 Q 2^-24 (the project's
     bound for a Q-term fp32 running sum), and >= 99.9 % of the picks equal float64's (the project's figure);
  4. frequencies: every class whose expected count n p >= 16 is within 6 standard errors sqrt(n p (1 - p)), the classes
     below 16 pooled into one bin; such a class is also seen at least once (p(never) <= e^-16), so a kept tie group is
     seen in all its members; a bin of probability 0 or 1 is met exactly;
  5. k = 1 on a tied maximum picks members of the top group only, and each of them.
Also: k = Q, k = Q + 5 and p = 1.0 are "off" to the bit; a free run from an RF-long prompt, in one launch and in three
uneven ones, repeats the teacher-forced picks (the logits do not depend on the history); a non-zero context changes
neither logits nor picks.

RESULTS
  One MI355X figure exists: with thread 0 of GENERIC's chooser summing in fp32 (as it did), the first row to fail was
  GENERIC G Q = 1000 five-model-T1-k0-p1: picks equal to float64's on 0.99854 of 4800 draws (7 differ), under check
  3's 99.9 %, with no pick outside the kept set, worst band excess 1.72e-06 (0.007 eps), 111 distinct classes, worst
  z 1.25.  planted_logits.emulate_draws with an fp32 running sum gives the same 0.99854 on that row, and 0.9948 ..
  0.9985 on eight GENERIC rows at Q = 1000 and 1024 (five at T = 1 and T = 1e4 untruncated, reference p = 0.3, straddle
  p = 0.999 and (9, 0.5)): a serial fp32 sum of ~1000 terms rounds the same way term after term, and 1000 band edges
  lie within that drift of a uniform.  The kernel was fixed, not the bound: thread 0 now forms total, target and
  running sum in double (csrc/generate.hip); the emulation, restated the same way, equals
  float64's pick on every draw of all GENERIC rows.
  UNVERIFIED on an MI355X: no run of this file with the fixed library could be made, nor of the two mutations
  (`>= theta` -> `> theta` where dropped classes are zeroed, `>= top_k` -> `> top_k` in the count, each in
  truncate_weights and truncate_weights_lds).  Wall time, worst band excess and equal-pick share per kernel, and the
  mutation counts are therefore NOT recorded here.  On the CPU (tests/test_planted_logits_host.py): checks 1 - 5 hold
  on float64's own picks for all 320 rows (so the frequency bins hold for this file's seed) and on the emulation (no
  pick outside the kept set, no kept class unseen); under the two mutations the emulation fails checks 2 / 4 / 5 on
  204 and 41 of the 320 rows, in every run.
"""
import functools

import numpy as np
import pytest
import torch

import planted_logits as P
import sampling_reference as R
import truncation_reference as TR
from helpers import synthetic_indices
from movenet_amd import _native as N
from movenet_amd.utils.weights import make_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 77
VARIANTS = {"GENERIC": N.GEN_GENERIC, "STREAM": N.GEN_STREAM, "PIPE": N.GEN_PIPE, "FOLD": N.GEN_FOLD,
            "PIPE_F16": N.GEN_PIPE_F16}
RUN_IDS = [f"{v}-{s}-Q{Q}" for v, s, Q, _, _ in P.RUNS]


@functools.lru_cache(maxsize=None)
def _weights(shape, Q):
    return {k: v.to(DEV) for k, v in make_state_dict(**P.shape_config(shape, Q), seed=3, gain=2.0, head_gain=6.0).items()}


@functools.lru_cache(maxsize=None)
def _planted(shape, Q, design):
    return P.plant(_weights(shape, Q), P.design(design, Q))


def _gen(variant, shape, Q, B, n_total, row, seed=SEED, context=None):
    from movenet_amd.generation import RingGenerator
    g = RingGenerator(**P.shape_config(shape, Q), state_dict=_planted(shape, Q, row.design), batch=B, n_total=n_total,
                      device=DEV, variant=VARIANTS[variant], temperature=row.T, seed=seed, sampling=row.rule,
                      top_k=row.k, top_p=row.p, context=context)
    with torch.cuda.device(g.device):
        assert g.lib.mvn_gen_variant(g.dims, VARIANTS[variant], B) == VARIANTS[variant] == g.variant
    return g


def _rf(shape, Q):
    return N.check(N.lib().mvn_receptive_fields(N.make_dims(**P.shape_config(shape, Q))), "mvn_receptive_fields")


def _teacher_forced(variant, shape, Q, B, n_new, row, context=None):
    """(picks (B, n_new) for times rf .. rf + n_new - 1, logits (B, n_new, Q)) of one teacher-forced run, as numpy."""
    rf = _rf(shape, Q)
    g = _gen(variant, shape, Q, B, rf + n_new, row, context=context)
    hist = synthetic_indices(B, rf + n_new, Q, 4321).to(DEV)
    choices, logits = g.teacher_forced(hist, logits_t0=rf)
    g.check_errors()
    return choices[:, rf:].cpu().numpy(), logits.cpu().numpy()


def _uniforms(seed, rf, B, n_new):
    """philox_uniform(seed, u, b) for u = rf .. rf + n_new - 1, b = 0 .. B - 1, as (B, n_new)."""
    return R.philox_uniform(seed, np.arange(rf, rf + n_new)[None, :], np.arange(B)[:, None])


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _check_run(picks, logits, Q, row, uniform, what):
    """Checks 1 - 5 of this file's header on every draw of a run."""
    planted = P.design(row.design, Q)
    n = picks.size
    # 1. the logits, to the bit
    assert logits.shape == picks.shape + (Q,)
    wrong = _bits(logits) != _bits(planted)
    assert not wrong.any(), f"{what}: {wrong.sum()} of {wrong.size} returned logits differ from the planted bias"
    assert picks.min() >= 0 and picks.max() < Q, f"{what}: picks outside [0, {Q})"
    # float64, once: every step has the same logits
    w = P.weights64(planted, row.rule, row.T)
    kept = TR.kept_set(w, row.k, row.p)
    cdf = TR.truncated_cdf(w, kept)
    prob = np.diff(cdf, prepend=0.0)
    cdf_all = np.broadcast_to(cdf, picks.shape + (Q,))
    # 2. the kept set
    outside = ~kept[picks]
    # 3. the band and float64's own pick
    eps = 4 * Q * 2.0 ** -24
    excess = R.band_excess(picks, cdf_all, uniform)
    want = R.inverse_cdf_picks(cdf_all, uniform)
    same = (picks == want).mean()
    # 4. frequencies
    counts = np.bincount(picks.ravel(), minlength=Q).astype(np.float64)
    small = n * prob < 16
    pb = np.append(prob[~small], prob[small].sum())
    fb = np.append(counts[~small], counts[small].sum()) / n
    sure = (pb <= 0) | (pb >= 1)
    z = np.zeros_like(pb)
    z[~sure] = np.abs(fb - pb)[~sure] / np.sqrt(pb * (1 - pb) / n)[~sure]
    print(f"EDGE {what}: kept {kept.sum()} of {Q}, picks outside the kept set {outside.sum()}; worst excess over the "
          f"float64 band {excess.max():.3g} (eps {eps:.3g}); equal to float64's pick on {same:.5f} of {n} draws; "
          f"{len(np.unique(picks))} distinct classes, {(~small).sum()} with n p >= 16, worst z {z.max():.2f}")
    assert not outside.any(), (f"{what}: {outside.sum()} of {n} picks outside the kept set, classes "
                               f"{np.unique(picks[outside]).tolist()[:12]}")
    assert (excess < eps).all(), (f"{what}: {(excess >= eps).sum()} of {n} draws outside the float64 band of their "
                                  f"pick, worst by {excess.max():.3g}")
    assert same >= 0.999, f"{what}: picks equal to float64's on {same:.5f} of {n} draws"
    assert (z < 6).all(), f"{what}: bins {np.nonzero(z >= 6)[0].tolist()} are {z[z >= 6].round(1).tolist()} standard errors out"
    assert np.array_equal(fb[sure], pb[sure]), f"{what}: a bin of probability 0 or 1 holds {fb[sure].tolist()}"
    unseen = np.nonzero(~small & (counts == 0))[0]
    assert unseen.size == 0, f"{what}: kept classes {unseen.tolist()} (expected count >= 16) were never drawn"
    # 5. k = 1: the tied maximum, all of it and nothing else
    if row.k == 1:
        top = np.nonzero(planted == planted.max())[0]
        assert np.unique(picks).tolist() == top.tolist(), f"{what}: k = 1 drew {np.unique(picks).tolist()}, top group {top.tolist()}"
    return excess.max(), same


# ---- 1 - 5. every row of the table -----------------------------------------------------------------------------
_TABLE = P.table()


@pytest.mark.parametrize("variant,shape,Q,B,n_new,row", _TABLE,
                         ids=[f"{v}-{s}-Q{Q}-{P.row_id(r)}" for v, s, Q, _, _, r in _TABLE])
def test_planted_row(variant, shape, Q, B, n_new, row):
    picks, logits = _teacher_forced(variant, shape, Q, B, n_new, row)
    _check_run(picks, logits, Q, row, _uniforms(SEED, _rf(shape, Q), B, n_new), f"{variant} {shape} Q={Q} {P.row_id(row)}")


# ---- off means off -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape,Q,B,n_new", P.RUNS, ids=RUN_IDS)
def test_off_knobs_draw_the_untruncated_run_to_the_bit(variant, shape, Q, B, n_new):
    n_new = 200
    design = "untied" if Q == 2 else "five"
    for rule in ("model", "reference"):
        base, logits = _teacher_forced(variant, shape, Q, B, n_new, P.Row(design, rule, 1.0, 0, 1.0))
        assert len(np.unique(base)) > 1
        for k in (Q, Q + 5):
            picks, again = _teacher_forced(variant, shape, Q, B, n_new, P.Row(design, rule, 1.0, k, 1.0))
            assert np.array_equal(picks, base), f"{rule}: top_k = {k}, top_p = 1.0 is not off"
            assert np.array_equal(_bits(again), _bits(logits))
        # (and the knobs do reach the kernel: k = 1 draws differently)
        picks, _ = _teacher_forced(variant, shape, Q, B, n_new, P.Row(design, rule, 1.0, 1, 1.0))
        assert not np.array_equal(picks, base)


# ---- the logits do not depend on the history: neither do the picks -----------------------------------------------
@pytest.mark.parametrize("run", P.HISTORY_RUNS, ids=[RUN_IDS[i] for i in P.HISTORY_RUNS])
def test_free_run_repeats_the_teacher_forced_picks(run):
    variant, shape, Q, B, _ = P.RUNS[run]
    row, rf, n_new = P.HISTORY_ROW, _rf(shape, Q), 60
    forced, logits = _teacher_forced(variant, shape, Q, B, n_new, row)
    _check_run(forced, logits, Q, row, _uniforms(SEED, rf, B, n_new), f"{variant} {shape} Q={Q} history row")
    prompt = synthetic_indices(B, rf, Q, 99).to(DEV)
    for chunks in ((n_new,), (7, 1, n_new - 8)):
        g = _gen(variant, shape, Q, B, rf + n_new, row)
        g.prime(prompt)
        assert g.n_given == rf
        for c in chunks:
            g.advance(c)
        g.check_errors()
        assert torch.equal(g.samples[:, :rf].cpu(), prompt.cpu().to(torch.int32))
        assert np.array_equal(g.samples[:, rf:].cpu().numpy(), forced), f"{variant}: launches of {chunks}"


@pytest.mark.parametrize("run", P.CONDITIONED_RUNS, ids=[RUN_IDS[i] for i in P.CONDITIONED_RUNS])
def test_context_changes_neither_logits_nor_picks(run):
    variant, shape, Q, B, _ = P.RUNS[run]
    row, rf, n_new = P.HISTORY_ROW, _rf(shape, Q), 120
    C = P.shape_config(shape, Q)["residual_channels"]
    ctx = torch.randn(B, C, rf + n_new, generator=torch.Generator().manual_seed(5)).to(DEV)
    plain, logits = _teacher_forced(variant, shape, Q, B, n_new, row)
    picks, again = _teacher_forced(variant, shape, Q, B, n_new, row, context=ctx)
    _check_run(picks, again, Q, row, _uniforms(SEED, rf, B, n_new), f"{variant} {shape} Q={Q} conditioned")
    assert np.array_equal(picks, plain) and np.array_equal(_bits(again), _bits(logits))
