"""GPU: the loss kernels under the "model" rule (mvn_softmax_ce_forward_ex / _backward_ex with MVN_LOSS_MODEL) through
the C ABI, at the edges of their dispatch, against the float64 restatement of tests/loss_rule_reference.py.

What the rule may and may not change: the probabilities written in place and the accuracy counts are the reference
rule's, bit for bit; the loss of a column is logsumexp(logits) - logits[target]; the gradient is
scale * upstream * (p - onehot) into the same padded window.  Both forward forms (the column form, Q <= 256 with
padding rows; one thread per column, Q > 256 or rows past the 32-bit offset limit), column counts that are no multiple
of 64, 256 or 4, windows that start off a 16-byte boundary, logits spread past sm_exp's underflow cut, exact ties, targets
out of range, an unknown rule, and MVN_LOSS_REFERENCE through the _ex calls against the plain entry points."""
import pytest
import torch

import loss_rule_reference as R
from helpers import first_bad_row, long_row_lengths
from movenet_amd import _native as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -1234.5
# elementwise fp32 outputs against float64: max |err| / max |ref| (test_loss_kernels_gpu.py's bound)
TOL = 2e-5
LOSS_TOL = 1e-5   # relative, on the summed loss (the same file's bound for the reference rule)


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _logits(B, Q, S, seed, spread=4.0, ties=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Q, S, generator=g) * spread
    tg = torch.randint(0, Q, (B, S), generator=g)
    if ties:
        # every third column: the maximum taken by several classes, in different 64-row waves when Q allows it;
        # the target is the LAST of them, so an accuracy that takes any maximum but the first one counts it
        rows = [r for r in (1, 70, 140, 200, 256) if r < Q] if Q > 8 else [0, Q - 1]
        top = x.amax(1) + 1.0
        for s in range(0, S, 3):
            for r in rows:
                x[:, r, s] = top[:, s]
            tg[:, s] = rows[-1]
    return x.to(DEV), tg.to(DEV)


def _err(got, want):
    return ((got.double() - want).abs().max() / want.abs().max().clamp_min(1e-30)).item()


def _parts(B, S, fill=0):
    parts = max(N.lib().mvn_ce_parts(B, S), 1)
    return (torch.full((parts,), float(fill), dtype=torch.float32, device=DEV),
            torch.full((parts,), int(fill), dtype=torch.int32, device=DEV))


def forward_plain(x, tg):
    B, Q, S = x.shape
    y = x.clone()
    lp, cp = _parts(B, S)
    N.check(N.lib().mvn_softmax_ce_forward(y.data_ptr(), tg.data_ptr(), B, Q, S, lp.data_ptr(), cp.data_ptr(),
                                           _stream()), "mvn_softmax_ce_forward")
    return y, lp, cp


def forward_ex(x, tg, rule):
    B, Q, S = x.shape
    y = x.clone()
    lp, cp = _parts(B, S)
    N.check(N.lib().mvn_softmax_ce_forward_ex(y.data_ptr(), tg.data_ptr(), B, Q, S, lp.data_ptr(), cp.data_ptr(),
                                              rule, _stream()), "mvn_softmax_ce_forward_ex")
    return y, lp, cp


def backward_ex(p, tg, scale, upstream, ld, col0, cols, rule):
    B, Q, S = p.shape
    d = torch.full((B, Q, ld), SENTINEL, dtype=torch.float32, device=DEV)
    N.check(N.lib().mvn_softmax_ce_backward_ex(p.data_ptr(), tg.data_ptr(), B, Q, S, scale,
                                               None if upstream is None else upstream.data_ptr(), d.data_ptr(),
                                               Q * ld, ld, col0, cols, rule, _stream()), "mvn_softmax_ce_backward_ex")
    return d


def _window(S):
    col0, cols = 5, S + 37
    return col0, cols, col0 + cols + 22


# Q: 2 and 100 (column form with padding rows), 256 (column form, none), 257 and 300 (one thread per column);
# S: 1, not a multiple of 64, not a multiple of 256
@pytest.mark.parametrize("Q", [2, 100, 256, 257, 300])
@pytest.mark.parametrize("S", [1, 333, 700])
def test_model_rule_forward_and_backward_vs_float64(Q, S):
    B = 2
    x, tg = _logits(B, Q, S, seed=Q * 1000 + S)
    y0, _, cp0 = forward_plain(x, tg)
    y, lp, cp = forward_ex(x, tg, N.LOSS_MODEL)
    assert torch.equal(y, y0)                      # the same probabilities, bit for bit
    assert int(cp.sum()) == int(cp0.sum())         # ... and the same accuracy count
    loss, loss64 = lp.double().sum().item(), R.model_loss_columns(x, tg).sum().item()
    print(f"Q {Q} S {S}: loss {loss:.6f} float64 {loss64:.6f} rel {abs(loss - loss64) / loss64:.2e}")
    assert abs(loss - loss64) < LOSS_TOL * loss64
    # backward into a padded window: columns [col0, col0 + cols) of rows of ld, cols > S (the extra ones zeroed),
    # everything outside the window untouched; scale and upstream multiply
    col0, cols, ld = _window(S)
    scale, up = 1.0 / (B * S), torch.tensor([2.5], device=DEV)
    p64 = R.model_probs(x)
    for upstream, factor in ((None, scale), (up, 2.5 * scale)):
        d = backward_ex(y, tg, scale, upstream, ld, col0, cols, N.LOSS_MODEL)
        e = _err(d[:, :, col0:col0 + S], R.model_dlogit(p64, tg, factor))
        print(f"  upstream {None if upstream is None else 2.5}: gradient err {e:.2e}")
        assert e < TOL, upstream
        assert bool((d[:, :, col0 + S:col0 + cols] == 0).all())
        assert bool((d[:, :, :col0] == SENTINEL).all()) and bool((d[:, :, col0 + cols:] == SENTINEL).all())


@pytest.mark.parametrize("Q", [256, 257])
def test_model_rule_exp_underflow_spread(Q):
    """logits spread 40 (about 240 apart in a column of 256): exponentials below sm_exp's cut are exactly 0"""
    B, S = 2, 200
    x, tg = _logits(B, Q, S, seed=5, spread=40.0)
    y, lp, _ = forward_ex(x, tg, N.LOSS_MODEL)
    assert bool((y == 0).any()) and bool(torch.isfinite(y).all())
    loss, loss64 = lp.double().sum().item(), R.model_loss_columns(x, tg).sum().item()
    print(f"Q {Q}: loss {loss:.4f} float64 {loss64:.4f}")
    assert bool(torch.isfinite(lp).all()) and abs(loss - loss64) < LOSS_TOL * loss64
    scale = 1.0 / (B * S)
    d = backward_ex(y, tg, scale, None, S, 0, S, N.LOSS_MODEL)
    assert bool(torch.isfinite(d).all()) and _err(d, R.model_dlogit(R.model_probs(x), tg, scale)) < TOL
    # an underflowed class: exactly -scale where it is the target, exactly 0 elsewhere
    hot = R.onehot(tg, Q).bool()
    under = y == 0
    assert bool((under & hot).any()) and bool((under & ~hot).any())
    assert bool((d[under & hot] == -torch.tensor(scale, dtype=torch.float32).item()).all())
    assert bool((d[under & ~hot] == 0).all())


@pytest.mark.parametrize("Q", [2, 100, 256, 257])
def test_model_rule_counts_ties_as_the_reference_rule_does(Q):
    B, S = 2, 333
    x, tg = _logits(B, Q, S, seed=99 + Q, ties=True)
    y0, _, cp0 = forward_plain(x, tg)
    y, _, cp = forward_ex(x, tg, N.LOSS_MODEL)
    assert int(((y == y.amax(1, keepdim=True)).sum(1) > 1).sum()) >= B * (S // 3)  # the ties survive the softmax
    assert torch.equal(cp, cp0) and torch.equal(y, y0)
    assert int(cp.sum()) == int((y.cpu().argmax(1) == tg.cpu()).sum())  # first maximum: torch.argmax's rule


@pytest.mark.parametrize("Q", [100, 300])
def test_model_rule_clamps_targets_out_of_range(Q):
    B, S = 2, 333
    x, tg = _logits(B, Q, S, seed=11 + Q)
    wild = tg.clone()
    wild[:, 0::7], wild[:, 3::7] = -3, Q + 5
    clamped = wild.clamp(0, Q - 1)
    ya, lpa, cpa = forward_ex(x, wild, N.LOSS_MODEL)
    yb, lpb, cpb = forward_ex(x, clamped, N.LOSS_MODEL)
    assert torch.equal(ya, yb) and torch.equal(lpa, lpb) and torch.equal(cpa, cpb)
    loss64 = R.model_loss_columns(x, clamped).sum().item()
    assert abs(lpa.double().sum().item() - loss64) < LOSS_TOL * loss64
    col0, cols, ld = _window(S)
    da = backward_ex(ya, wild, 0.5, None, ld, col0, cols, N.LOSS_MODEL)
    db = backward_ex(ya, clamped, 0.5, None, ld, col0, cols, N.LOSS_MODEL)
    assert torch.equal(da, db)
    # and the reference rule, through the same calls, clamps alike
    _, lpr, cpr = forward_ex(x, wild, N.LOSS_REFERENCE)
    _, lpc, cpc = forward_ex(x, clamped, N.LOSS_REFERENCE)
    assert torch.equal(lpr, lpc) and torch.equal(cpr, cpc) and torch.equal(cpr, cpa)


def test_model_rule_past_the_offset_limit():
    """one sequence of Q = 256 rows so long that the tail of the last row lies past 2^31 bytes: the column form
    gives way to the form with 64-bit addresses; every row of the loss and of the gradient must still be right"""
    Q, B = 256, 1
    S = long_row_lengths(Q)["tail"]
    g = torch.Generator(device=DEV).manual_seed(17)
    x = torch.randn(B, Q, S, generator=g, device=DEV) * 4.0
    tg = torch.randint(0, Q, (B, S), generator=g, device=DEV)
    y, lp, cp = forward_ex(x, tg, N.LOSS_MODEL)
    scale = 1.0 / S
    d = torch.empty_like(y)
    N.check(N.lib().mvn_softmax_ce_backward_ex(y.data_ptr(), tg.data_ptr(), B, Q, S, scale, None, d.data_ptr(), Q * S,
                                               S, 0, S, N.LOSS_MODEL, _stream()), "mvn_softmax_ce_backward_ex")
    # the last row, where an offset past the limit shows first: its tail columns must not have been dropped
    assert bool((y[0, Q - 1, -64:] > 0).all()) and bool((d[0, Q - 1, -64:] != 0).any())
    bad = first_bad_row(Q, S)
    step = 1 << 18  # float64 references column block by column block
    loss64, worst = 0.0, 0.0
    for c0 in range(0, S, step):
        c1 = min(S, c0 + step)
        xs, ts = x[:, :, c0:c1], tg[:, c0:c1]
        loss64 += R.model_loss_columns(xs, ts).sum().item()
        worst = max(worst, _err(d[:, :, c0:c1], R.model_dlogit(R.model_probs(xs), ts, scale)))
    loss = lp.double().sum().item()
    print(f"S {S}: loss {loss:.3f} float64 {loss64:.3f}, gradient err {worst:.2e}, first row past the limit {bad}")
    assert worst < TOL, (bad, worst)
    # (fp32 sums of a workgroup's columns, added in float64 here: the bound does not grow with S)
    assert abs(loss - loss64) < LOSS_TOL * loss64, (loss, loss64)
    assert int(cp.sum()) == int((y.argmax(1) == tg).sum())
    del x, y, d
    torch.cuda.empty_cache()


def test_unknown_rule_is_refused_and_touches_nothing():
    B, Q, S = 2, 100, 333
    _, tg = _logits(B, Q, S, seed=3)
    lib = N.lib()
    y = torch.full((B, Q, S), float("nan"), device=DEV)
    lp, cp = _parts(B, S, fill=-7)
    rc = lib.mvn_softmax_ce_forward_ex(y.data_ptr(), tg.data_ptr(), B, Q, S, lp.data_ptr(), cp.data_ptr(), 7, _stream())
    assert rc == N.MVN_ERR_BAD_ARG and "mvn_softmax_ce_forward_ex" in N.last_error()
    d = torch.full((B, Q, S + 64), float("nan"), device=DEV)
    rc = lib.mvn_softmax_ce_backward_ex(y.data_ptr(), tg.data_ptr(), B, Q, S, 1.0, None, d.data_ptr(), Q * (S + 64),
                                        S + 64, 5, S + 37, 7, _stream())
    assert rc == N.MVN_ERR_BAD_ARG and "mvn_softmax_ce_backward_ex" in N.last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(d).all())
    assert bool((lp == -7).all()) and bool((cp == -7).all())


@pytest.mark.parametrize("Q", [100, 257])
def test_reference_rule_through_the_ex_calls_is_the_plain_calls(Q):
    B, S = 2, 333
    x, tg = _logits(B, Q, S, seed=21 + Q)
    y0, lp0, cp0 = forward_plain(x, tg)
    y, lp, cp = forward_ex(x, tg, N.LOSS_REFERENCE)
    assert torch.equal(y, y0) and torch.equal(lp, lp0) and torch.equal(cp, cp0)
    col0, cols, ld = _window(S)
    up = torch.tensor([2.5], device=DEV)
    d0 = torch.full((B, Q, ld), SENTINEL, dtype=torch.float32, device=DEV)
    N.check(N.lib().mvn_softmax_ce_backward(y0.data_ptr(), tg.data_ptr(), B, Q, S, 0.25, up.data_ptr(), d0.data_ptr(),
                                            Q * ld, ld, col0, cols, _stream()), "mvn_softmax_ce_backward")
    d = backward_ex(y, tg, 0.25, up, ld, col0, cols, N.LOSS_REFERENCE)
    assert torch.equal(d, d0)
    # and the two rules do differ: the model rule's loss is not confined to [ln Q - 1, ln Q]
    _, lpm, _ = forward_ex(x, tg, N.LOSS_MODEL)
    assert lpm.sum().item() > 1.5 * lp.sum().item()
