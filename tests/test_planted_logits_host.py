"""CPU: the planted-logits table of tests/planted_logits.py is DECIDABLE -- on every row the kept set that
include/movenet_hip.h prescribes does not depend on rounding, so tests/test_sampling_edges_gpu.py exempts no step.

For every row (design, rule, T, top_k, top_p) of the table:
  (a) the float64 kept set (tests/truncation_reference.py) is a union of whole tie groups;
  (b) it is the same at p (1 - SUM_EPS) and p (1 + SUM_EPS), SUM_EPS = 2^-14;
  (c) the weights as fp32 forms them (numpy float32 exp of the float32 argument, both rules) give the same kept set on
      every class of positive fp32 weight (a class whose fp32 weight underflowed to zero cannot be drawn);
  (d) the threshold group leads the next lower group of positive fp32 weight by at least 2^-10 relatively -- far above
      TIE_EPS = 2^-18, so no hardware exp reorders them.
A row that fails one of them is deleted from the table (planted_logits.DELETED), never skipped at run time; this file
fails if such a row is put back, p = 1 - 2^-24 for one."""
import numpy as np
import pytest
import torch

import planted_logits as P
import sampling_reference as R
import truncation_reference as TR
from movenet_amd.utils.weights import make_state_dict

TABLE = P.table()


def test_every_row_of_the_table_is_decidable():
    assert len(TABLE) > 250
    seen = set()
    for variant, shape, Q, B, n_new, row in TABLE:
        if (Q, row) in seen:
            continue
        seen.add((Q, row))
        found = P.defects(P.design(row.design, Q), row.rule, row.T, row.k, row.p)
        assert not found, f"Q = {Q}, {P.row_id(row)}: {found}"
        assert 0 <= row.k < Q and 0.0 < row.p <= 1.0 and row.T > 0  # (k >= Q is "off": the GPU file's own test)


def test_the_history_row_is_decidable_where_it_runs():
    assert {P.RUNS[i][0] for i in P.HISTORY_RUNS} == {"GENERIC", "STREAM", "PIPE", "FOLD", "PIPE_F16"}
    assert [P.RUNS[i][0] for i in P.CONDITIONED_RUNS] == ["GENERIC", "STREAM", "FOLD"]
    for i in P.HISTORY_RUNS + P.CONDITIONED_RUNS:
        Q, row = P.RUNS[i][2], P.HISTORY_ROW
        assert P.defects(P.design(row.design, Q), row.rule, row.T, row.k, row.p) == []
        assert TR.kept_set(P.weights64(P.design(row.design, Q), row.rule, row.T), row.k, row.p).sum() == 16


def test_deleted_rows_are_undecidable_and_absent():
    assert P.DELETED
    for (Q, row), reason in P.DELETED.items():
        found = P.defects(P.design(row.design, Q), row.rule, row.T, row.k, row.p)
        assert found and found[0][:3] == reason[:3], (Q, row, found)
        assert all((q, r) != (Q, row) for _, _, q, _, _, r in TABLE)


@pytest.mark.parametrize("Q,name", [(2, "untied"), (64, "five"), (100, "five"), (256, "straddle"), (1024, "five")])
def test_p_one_minus_2_to_the_minus_24_is_rejected(Q, name):
    """At T = 0.02 everything below the top group weighs under 2e-22 of it: p (1 - SUM_EPS) keeps the top group alone,
    p (1 + SUM_EPS) >= 1 is "off" and keeps every class."""
    found = P.defects(P.design(name, Q), "model", 0.02, 0, 1.0 - 2.0 ** -24)
    assert any(f.startswith("(b)") for f in found), found


def test_other_undecidable_rows_are_rejected():
    five = P.design("five", 256)
    # (d): at T = 1e4 five's groups are 1e-4 apart
    assert any(f.startswith("(d)") for f in P.defects(five, "model", 1e4, 3, 1.0))
    # (b): p S on the edge of a group -- the top group of five holds exactly its share
    w = TR.model_weights(five, 1.0)
    share = w[five == 3.0].sum() / w.sum()
    assert any(f.startswith("(b)") for f in P.defects(five, "model", 1.0, 0, float(share)))
    # (c): at T = 0.02, k = 9 fp32 keeps MORE than float64 (the third group underflows, the 9th largest weight is 0) --
    # on classes of zero weight only, which cannot be drawn: (c) allows it
    assert P.defects(five, "model", 0.02, 9, 1.0) == []
    kept64 = TR.kept_set(TR.model_weights(five, 0.02), 9)
    kept32 = TR.kept_set(P.weights32(five, "model", 0.02).astype(np.float64), 9)
    assert kept64.sum() == 16 and kept32.all()


def test_tie_groups_weigh_bit_equal_in_fp32_under_both_rules():
    for Q, name in [(2, "tied"), (64, "five"), (257, "five"), (256, "straddle"), (1000, "wide")]:
        logits = P.design(name, Q)
        for rule in ("model", "reference"):
            for T in P.TEMPERATURES:
                w = P.weights32(logits, rule, T)
                for g in P.groups(logits):
                    assert len(np.unique(w[g].view(np.uint32))) == 1, (Q, name, rule, T)


def test_designs_are_what_the_header_says():
    for Q in (64, 100, 128, 200, 256, 257, 1000, 1024):
        five = P.design("five", Q)
        assert five.dtype == np.float32 and five.shape == (Q,)
        assert [(float(five[g][0]), int(g.sum())) for g in P.groups(five)] == \
            list(P.FIVE_GROUPS) + [(P.FIVE_FLOOR, Q - 32)]
        assert np.array_equal(P.design("wide", Q), five * 10)
        s = P.design("straddle", Q)
        a = 63 if Q > 64 else 31
        assert np.nonzero(s == 3.0)[0].tolist() == [a, a + 1, Q - 1]
        assert Q == 64 or a // 64 != (a + 1) // 64  # two trips of the one-wave select's loop
        assert (a + 1) % 4 == 0  # the pair also sits in two lanes of the pipelined heads (4 classes per lane)
        assert [int(g.sum()) for g in P.groups(s)] == [3, 4, Q - 7]
    assert P.design("untied", 2).tolist() == [0.0, -1.0] and P.design("tied", 2).tolist() == [0.0, 0.0]


def test_designs_and_philox_are_deterministic():
    for name, Q in [("five", 100), ("wide", 1024), ("straddle", 257), ("untied", 2)]:
        first = P.design(name, Q)
        P._design.cache_clear()
        again = P.design(name, Q)
        assert first is not again and np.array_equal(first.view(np.uint32), again.view(np.uint32))
        first[:] = 9  # (a copy: the cached design is not touched)
        assert np.array_equal(P.design(name, Q), again)
    u = [R.philox_uniform(77, np.arange(8, 308)[None, :], np.arange(16)[:, None]) for _ in range(2)]
    assert np.array_equal(u[0], u[1]) and u[0].shape == (16, 300)
    assert (u[0] >= 0).all() and (u[0] < 1).all() and np.array_equal(u[0] * 2 ** 24, np.round(u[0] * 2 ** 24))
    assert 0.45 < u[0].mean() < 0.55 and len(np.unique(u[0])) > 4700
    assert [P.row_id(r[-1]) for r in P.table()] == [P.row_id(r[-1]) for r in TABLE]


def test_plant_zeroes_the_last_product_and_leaves_the_rest():
    cfg = P.shape_config("G", 100)
    sd = make_state_dict(**cfg, seed=3, gain=2.0, head_gain=6.0)
    logits = P.design("five", 100)
    planted = P.plant(sd, logits)
    assert set(planted) == set(sd)
    for key in sd:
        if key == "dense_conv.conv2.weight":
            assert planted[key].shape == sd[key].shape and not bool(planted[key].any()) and bool(sd[key].any())
        elif key == "dense_conv.conv2.bias":
            assert np.array_equal(planted[key].numpy().view(np.uint32), logits.view(np.uint32))
            assert planted[key].dtype == torch.float32
        else:
            assert planted[key] is sd[key]


def test_the_table_covers_what_it_must():
    runs = {(v, s, Q) for v, s, Q, _, _, _ in TABLE}
    assert {Q for v, _, Q in runs if v == "GENERIC"} == {2, 100, 200, 257, 1000, 1024}
    for v in ("STREAM", "PIPE", "FOLD"):
        assert {Q for w, _, Q in runs if w == v} >= {128, 256}
    assert ("FOLD", "S64", 64) in runs and ("PIPE_F16", "S128", 256) in runs
    for v, s, Q in runs:
        rows = [r for w, t, q, _, _, r in TABLE if (w, t, q) == (v, s, Q)]
        assert {r.T for r in rows if r.rule == "model" and r.k == 0 and r.p == 1.0} == set(P.TEMPERATURES)
        for T in (0.02, 1e4):  # one top-k and one top-p row at each extreme (Q = 2 at T = 1e4: top-p alone passes (d))
            assert any(r.T == T and r.p < 1.0 for r in rows)
            assert any(r.T == T and r.k > 0 for r in rows) or (Q == 2 and T == 1e4)
        assert any(r.rule == "reference" and r.k > 0 for r in rows)
        assert any(r.rule == "reference" and r.p < 1.0 for r in rows)
        assert 15 <= len(rows) <= 24
    # the knob rows at T = 1 and T = 0.25: every one of them runs somewhere, on both designs
    for Q in (100, 256):
        assert len(P.pool(Q)) == 52
    ran = {(r.design, r.T, r.k if r.k < 10 else "Q-1", r.p) for _, _, Q, _, _, r in TABLE if Q > 2}
    for row in P.pool(256):
        assert (row.design, row.T, row.k if row.k < 10 else "Q-1", row.p) in ran, row
    # a tied maximum under k = 1, thresholds inside a group and on its edge, the smallest p
    for v in {v for v, _, _ in runs}:
        rows = [r for w, _, Q, _, _, r in TABLE if w == v]
        assert any(r.k == 1 for r in rows) and any(r.p == 1e-6 for r in rows)
        assert any(r.design == "five" and r.k in (4, 9) for r in rows)
        assert any(r.design == "five" and r.k in (3, 8) for r in rows)


def _kept_set_findings(picks, Q, row):
    """Checks 2, 4 (never-drawn classes) and 5 of the GPU file on one run's picks."""
    planted = P.design(row.design, Q)
    w = P.weights64(planted, row.rule, row.T)
    kept = TR.kept_set(w, row.k, row.p)
    prob = np.diff(TR.truncated_cdf(w, kept), prepend=0.0)
    counts = np.bincount(picks.ravel(), minlength=Q)
    out = []
    if not kept[picks].all():
        out.append("a pick outside the kept set")
    if ((picks.size * prob >= 16) & (counts == 0)).any():
        out.append("a kept class never drawn")
    if row.k == 1 and np.unique(picks).tolist() != np.nonzero(planted == planted.max())[0].tolist():
        out.append("k = 1 did not draw the top group")
    return out


def test_an_emulated_fp32_select_passes_and_its_two_mutations_do_not():
    """numpy's restatement of the select (planted_logits.emulate_draws) on the table's own uniforms: as the header
    prescribes it, no row has a finding; with `>` for `>=` where dropped classes are zeroed, or in top-k's count, every
    run of the table has rows that do (`>` at the threshold: the rows whose threshold is positive; the count: the rows
    whose k ends on the edge of a tie group)."""
    failed = {1: {}, 2: {}}
    for i, (variant, shape, Q, B, n_new) in enumerate(P.RUNS):
        u = R.philox_uniform(77, np.arange(16, 16 + n_new)[None, :], np.arange(B)[:, None])
        for row in P.rows_of(i):
            planted = P.design(row.design, Q)
            assert _kept_set_findings(P.emulate_draws(planted, row, u), Q, row) == [], (Q, row)
            for m in (1, 2):
                if _kept_set_findings(P.emulate_draws(planted, row, u, mutation=m), Q, row):
                    failed[m].setdefault(i, []).append(row)
    for m in (1, 2):
        assert sorted(failed[m]) == list(range(len(P.RUNS))), (m, sorted(failed[m]))
    print({m: sum(len(v) for v in failed[m].values()) for m in (1, 2)})
