"""GPU: mvn_score_columns through the C ABI against the float64 restatement of tests/score_reference.py.

Shapes: the full cross product Q in {4, 64, 100, 128, 256, 300} x S in {1, 63, 64, 65, 257, 1001} x B in {1, 3} -- the
column form with and without padding rows and whole padding waves (Q <= 256), one thread per column (Q = 300), one and
several workgroups, odd S (rows off 16-byte boundaries) -- each at temperatures 0.5, 1 and 2 on logits randn x 4 and
randn x 40 (differences past sm_exp's -103 cut, columns so peaked that log(sum) needs log1p).

Bounds: logp and entropy within max|err| / max|ref| <= 2e-5 (the TOL of test_loss_rule_kernels_gpu.py, the project's
bound for these column kernels), seq_nll within 1e-5 relative (its LOSS_TOL), rank and seq_correct exact.  Every call
runs on sentinel-banded buffers with a NaN-filled scratch, leaves the logits bit-equal and is repeated once for
bit-equal results.

The column form addresses a sequence's tensor with 32-bit buffer offsets, so the 2^31-byte bound is crossed once
(helpers.long_row_lengths): just below it the column form runs at its largest offsets, just past it the 64-bit form.

Measured on an MI355X, worst error over the 72 shapes as a fraction of its bound: logp 0.006, entropy 0.028, seq_nll
0.20; at the offset limit logp 6.8e-8 and 1.0e-7 of max|ref|."""
import itertools
import math

import pytest
import torch

import score_reference as SR
from helpers import SENTINEL, _Guard, first_bad_row, long_row_lengths
from movenet_amd import _native as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-5        # elementwise fp32 outputs against float64: max |err| / max |ref|
NLL_TOL = 1e-5    # relative, on a sequence's summed log-likelihood
OUTPUTS = ("logp", "entropy", "rank", "seq_nll", "seq_correct")
worst = {"logp": 0.0, "entropy": 0.0, "seq_nll": 0.0}   # the largest error seen, as a fraction of its bound


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _logits(B, Q, S, seed, spread=4.0, ties=False):
    """test_loss_rule_kernels_gpu.py's _logits: with ``ties`` every third column has its maximum shared by classes in
    different 64-row groups, the target the LAST of them"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Q, S, generator=g) * spread
    tg = torch.randint(0, Q, (B, S), generator=g)
    rows = None
    if ties:
        rows = [r for r in (1, 70, 140, 200, 256) if r < Q] if Q > 8 else [0, Q - 1]
        top = x.amax(1) + 1.0
        for s in range(0, S, 3):
            for r in rows:
                x[:, r, s] = top[:, s]
            tg[:, s] = rows[-1]
    return x.to(DEV), tg.to(DEV), rows


def _err(got, want):
    finite = torch.isfinite(want)
    assert torch.equal(got.double()[~finite], want[~finite])           # -inf where the reference has -inf
    if not bool(finite.any()):
        return 0.0
    return ((got.double()[finite] - want[finite]).abs().max() / want[finite].abs().max().clamp_min(1e-300)).item()


def run(x, tg, temperature=1.0, want=OUTPUTS, guard=None, scratch_floats=None):
    """One call on banded buffers; returns (status, outputs dict -- EVERY buffer, sentinel-filled where not asked for)."""
    B, Q, S = x.shape
    lib = N.lib()
    guard = guard or _Guard()
    shapes = {"logp": ((B, S), torch.float32), "entropy": ((B, S), torch.float32), "rank": ((B, S), torch.int32),
              "seq_nll": ((B,), torch.float32), "seq_correct": ((B,), torch.int32)}
    out = {k: guard.new(shape, fill=SENTINEL if dt.is_floating_point else int(SENTINEL), name=k, dtype=dt)
           for k, (shape, dt) in shapes.items()}
    n = lib.mvn_score_scratch_floats(B, S) if scratch_floats is None else scratch_floats
    scratch = guard.new((max(n, 1),), fill=float("nan"), name="scratch")
    rc = lib.mvn_score_columns(x.data_ptr(), tg.data_ptr(), B, Q, S, temperature,
                               *[out[k].data_ptr() if k in want else None for k in OUTPUTS],
                               scratch.data_ptr(), n, _stream())
    guard.check("mvn_score_columns")
    return rc, out


def check_against_float64(x, tg, T, label):
    guard = _Guard()
    xin = guard.put(x, name="logits")                                  # (rows off the allocator's alignment for odd S)
    before = xin.clone()
    rc, got = run(xin, tg, T, guard=guard)
    assert rc == N.MVN_OK, N.last_error()
    assert torch.equal(xin.view(torch.int32), before.view(torch.int32))    # read only
    rc, again = run(xin, tg, T)
    assert rc == N.MVN_OK and all(torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)) for k in OUTPUTS)
    ref = SR.score(x, tg, T)
    e_lp, e_h = _err(got["logp"], ref["logp"]), _err(got["entropy"], ref["entropy"])
    ok = torch.isfinite(ref["seq_nll"])                                # (+inf where a target is masked: equal, not close)
    assert torch.equal(got["seq_nll"].double()[~ok], ref["seq_nll"][~ok])
    e_nll = ((got["seq_nll"].double() - ref["seq_nll"]).abs() / ref["seq_nll"].abs().clamp_min(1e-300))[ok]
    e_nll = e_nll.max().item() if bool(ok.any()) else 0.0
    print(f"{label} T {T}: logp {e_lp:.2e} entropy {e_h:.2e} seq_nll {e_nll:.2e}")
    for k, e, bound in (("logp", e_lp, TOL), ("entropy", e_h, TOL), ("seq_nll", e_nll, NLL_TOL)):
        worst[k] = max(worst[k], e / bound)
    assert e_lp <= TOL and e_h <= TOL and e_nll <= NLL_TOL, (label, T, e_lp, e_h, e_nll)
    assert torch.equal(got["rank"].long(), ref["rank"])
    assert torch.equal(got["seq_correct"].long(), ref["seq_correct"])
    return got, ref


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S", [1, 63, 64, 65, 257, 1001])
@pytest.mark.parametrize("Q", [4, 64, 100, 128, 256, 300])
def test_score_columns_vs_float64(Q, S, B):
    for spread in (4.0, 40.0):
        x, tg, _ = _logits(B, Q, S, seed=Q * 10000 + S * 10 + B, spread=spread)
        for T in (0.5, 1.0, 2.0):
            check_against_float64(x, tg, T, f"Q {Q} S {S} B {B} x{spread:g}")
    print("worst error so far, as a fraction of its bound:", {k: round(v, 4) for k, v in worst.items()})


@pytest.mark.parametrize("Q", [4, 100, 256, 300])
def test_planted_ties_rank_counts_the_earlier_equals(Q):
    B, S = 3, 257
    x, tg, rows = _logits(B, Q, S, seed=77 + Q, ties=True)
    for T in (0.5, 1.0, 2.0):
        got, _ = check_against_float64(x, tg, T, f"ties Q {Q}")
        tied = got["rank"][:, 0::3]
        assert bool((tied == len(rows) - 1).all()) and len(rows) >= 2       # the earlier equals, never 0
    # with the target the FIRST of the tied classes the column is correct: rank 0
    first = tg.clone()
    first[:, 0::3] = rows[0]
    rc, got = run(x, first)
    assert rc == N.MVN_OK and bool((got["rank"][:, 0::3] == 0).all())
    assert torch.equal(got["seq_correct"].long(), (got["rank"] == 0).sum(1))


@pytest.mark.parametrize("Q", [100, 256, 300])
def test_masked_classes_and_targets_out_of_range(Q):
    B, S = 3, 257
    x, tg, _ = _logits(B, Q, S, seed=5 + Q)
    g = torch.Generator().manual_seed(Q)
    mask = (torch.rand(B, Q, S, generator=g) < 0.3).to(DEV)
    hot = torch.zeros(B, Q, S, dtype=torch.bool, device=DEV).scatter_(1, tg[:, None], True)
    keep = x.argmax(1, keepdim=True)                                        # (never a whole column)
    mask = mask & ~hot & ~torch.zeros_like(hot).scatter_(1, keep, True)
    xm = x.masked_fill(mask, -math.inf)
    got, _ = check_against_float64(xm, tg, 1.0, f"masked Q {Q}")
    assert bool(torch.isfinite(got["logp"]).all()) and bool(torch.isfinite(got["entropy"]).all())
    # -inf on the target of every fifth column: logp = -inf there, the entropy stays finite
    xt = xm.clone()
    cols = torch.arange(0, S, 5, device=DEV)
    other = (tg[:, cols] + 1) % Q
    xt[:, :, cols] = xt[:, :, cols].scatter(1, other[:, None], 1.0)         # (a finite class besides the target)
    xt[:, :, cols] = xt[:, :, cols].scatter(1, tg[:, None, cols], -math.inf)
    got, _ = check_against_float64(xt, tg, 2.0, f"masked target Q {Q}")
    assert bool((got["logp"][:, cols] == -math.inf).all()) and bool(torch.isfinite(got["entropy"]).all())
    assert bool((got["seq_nll"] == math.inf).all())
    # targets out of range behave as clamped
    wild = tg.clone()
    wild[:, 0::7], wild[:, 3::7] = -3, Q + 5
    rc_a, a = run(x, wild, 0.5)
    rc_b, b = run(x, wild.clamp(0, Q - 1), 0.5)
    assert rc_a == rc_b == N.MVN_OK and all(torch.equal(a[k], b[k]) for k in OUTPUTS)


@pytest.mark.parametrize("Q,S", [(100, 257), (300, 65)])
def test_every_subset_of_outputs(Q, S):
    B = 3
    x, tg, _ = _logits(B, Q, S, seed=31 + Q)
    rc, full = run(x, tg, 0.5)
    assert rc == N.MVN_OK
    for r in range(len(OUTPUTS)):
        for want in itertools.combinations(OUTPUTS, r):
            rc, got = run(x, tg, 0.5, want=want)
            assert rc == N.MVN_OK, (want, N.last_error())
            for k in OUTPUTS:
                if k in want:
                    assert torch.equal(got[k].view(torch.int32), full[k].view(torch.int32)), (want, k)
                else:                                                       # not asked for: not written
                    assert bool((got[k] == (SENTINEL if got[k].is_floating_point() else int(SENTINEL))).all()), (want, k)


def test_bad_temperature_and_short_scratch_touch_nothing():
    B, Q, S = 3, 100, 257
    x, tg, _ = _logits(B, Q, S, seed=3)
    before = x.clone()
    need = N.lib().mvn_score_scratch_floats(B, S)
    for T, floats in ((0.0, None), (-1.0, None), (math.inf, None), (math.nan, None), (1.0, need - 1), (1.0, 0)):
        rc, got = run(x, tg, T, scratch_floats=floats)
        assert rc == N.MVN_ERR_BAD_ARG and "mvn_score_columns" in N.last_error(), (T, floats)
        for k in OUTPUTS:
            assert bool((got[k] == (SENTINEL if got[k].is_floating_point() else int(SENTINEL))).all()), (T, floats, k)
    assert torch.equal(x, before)
    # an empty sequence: nothing to read, zeros in the sums
    rc, got = run(torch.empty(B, Q, 0, device=DEV), torch.empty(B, 0, dtype=torch.int64, device=DEV))
    assert rc == N.MVN_OK and bool((got["seq_nll"] == 0).all()) and bool((got["seq_correct"] == 0).all())


@pytest.mark.parametrize("Q,S,ties", [(100, 333, False), (256, 700, False), (256, 333, True), (300, 333, False),
                                      (300, 333, True)])
def test_sums_are_the_loss_forwards(Q, S, ties):
    """On the same tensor the model rule's loss forward (mvn_softmax_ce_forward_ex, MVN_LOSS_MODEL) reports the mean of
    -logp and the number of rank-0 columns: sum(seq_nll) / (B S) within 1e-5 relative, sum(seq_correct) exactly."""
    B = 3
    x, tg, _ = _logits(B, Q, S, seed=200 + Q + S, ties=ties)
    rc, got = run(x, tg)
    assert rc == N.MVN_OK
    y = x.clone()
    parts = max(N.lib().mvn_ce_parts(B, S), 1)
    lp = torch.zeros(parts, dtype=torch.float32, device=DEV)
    cp = torch.zeros(parts, dtype=torch.int32, device=DEV)
    N.check(N.lib().mvn_softmax_ce_forward_ex(y.data_ptr(), tg.data_ptr(), B, Q, S, lp.data_ptr(), cp.data_ptr(),
                                              N.LOSS_MODEL, _stream()), "mvn_softmax_ce_forward_ex")
    loss = lp.double().sum().item() / (B * S)
    mine = got["seq_nll"].double().sum().item() / (B * S)
    print(f"Q {Q} S {S}: loss forward {loss:.7f}, score {mine:.7f}, rel {abs(mine - loss) / loss:.2e}")
    assert abs(mine - loss) <= 1e-5 * loss
    assert int(got["seq_correct"].sum()) == int(cp.sum())


@pytest.mark.parametrize("which", ["below", "tail"])
def test_at_the_offset_limit(which):
    """one sequence of Q = 256 rows whose last row ends just below 2^31 bytes (the column form at its largest 32-bit
    offsets) and one whose last row's tail lies past them (the form with 64-bit addresses): every column, the last
    row's tail included, must still be right"""
    Q, B = 256, 1
    S = long_row_lengths(Q)[which]
    g = torch.Generator(device=DEV).manual_seed(17)
    x = torch.randn(B, Q, S, generator=g, device=DEV) * 4.0
    tg = torch.randint(0, Q, (B, S), generator=g, device=DEV)
    tg[:, -64:] = Q - 1                                      # the last row's tail carries the targets' logits
    lib = N.lib()
    logp = torch.empty(B, S, device=DEV)
    rank = torch.empty(B, S, dtype=torch.int32, device=DEV)
    nll, ok = torch.empty(B, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV)
    n = lib.mvn_score_scratch_floats(B, S)
    scratch = torch.full((n,), float("nan"), device=DEV)
    N.check(lib.mvn_score_columns(x.data_ptr(), tg.data_ptr(), B, Q, S, 1.0, logp.data_ptr(), None, rank.data_ptr(),
                                  nll.data_ptr(), ok.data_ptr(), scratch.data_ptr(), n, _stream()), "mvn_score_columns")
    step = 1 << 18  # float64 references column block by column block
    nll64, correct, e_max, ref_max = 0.0, 0, 0.0, 0.0
    for c0 in range(0, S, step):
        c1 = min(S, c0 + step)
        ref = SR.score(x[:, :, c0:c1], tg[:, c0:c1], 1.0)
        nll64 += ref["seq_nll"].sum().item()
        correct += int(ref["seq_correct"].sum())
        e_max = max(e_max, (logp[:, c0:c1].double() - ref["logp"]).abs().max().item())
        ref_max = max(ref_max, ref["logp"].abs().max().item())
        assert torch.equal(rank[:, c0:c1].long(), ref["rank"]), (c0, first_bad_row(Q, S))
        del ref
    print(f"{which}: S {S}, first row past the limit {first_bad_row(Q, S)}, logp err {e_max / ref_max:.2e}, "
          f"seq_nll {nll.item():.3f} float64 {nll64:.3f}")
    assert e_max <= TOL * ref_max
    assert abs(nll.double().item() - nll64) <= NLL_TOL * nll64 and int(ok) == correct
    del x, logp, rank
    torch.cuda.empty_cache()
