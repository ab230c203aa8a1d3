"""GPU: the loss and score kernels with a per-sequence column count (mvn_softmax_ce_forward_len / _backward_len,
mvn_score_columns_len) through the C ABI, on planted buffers with sentinel bands.

B = 3 sequences of S = 130 columns (two full 64-column tiles and one of two columns) at Q = 64, 200, 256 -- the
64-column form -- and S = 70 at Q = 257, one thread per column; both loss rules; every sequence full, one empty / one
cut inside the second tile / one full, cuts one column either side of a tile edge, and counts outside [0, S] for the
kernel's clamp.  Held to: the _ex calls and mvn_score_columns, bit for bit, where every column counts (and with
valid = NULL); tests/masked_reference.py in float64 under the bounds the unmasked kernels are held to
(test_loss_rule_kernels_gpu.py: LOSS_TOL on the summed loss, TOL on the gradient; test_score_gpu.py: TOL, NLL_TOL);
exact counts; NaN and +inf in the logits of columns that do not count changing nothing; two calls, the same bits."""
import math

import pytest
import torch

import masked_reference as MR
from helpers import SENTINEL, _Guard
from movenet_amd import _native as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-5        # test_loss_rule_kernels_gpu.py: elementwise fp32 outputs against float64, max |err| / max |ref|
LOSS_TOL = 1e-5   # the same file: relative, on the summed loss
NLL_TOL = 1e-5    # test_score_gpu.py: relative, on a sequence's summed log-likelihood
B = 3
SHAPES = [(64, 130), (200, 130), (256, 130), (257, 70)]
RULES = {"reference": N.LOSS_REFERENCE, "model": N.LOSS_MODEL}


def _valid_sets(S):
    return [[S, S, S], [0, S // 2, S], [1, 64, S - 1], [S + 7, -3, 65]]


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _logits(Q, S, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, Q, S, generator=g) * 4.0).to(DEV), torch.randint(0, Q, (B, S), generator=g).to(DEV)


def _bits(t):
    return t.view(torch.int32)


def _dev_valid(valid):
    return None if valid is None else torch.tensor(valid, dtype=torch.int32, device=DEV)


def _plant(x, valid, value):
    """``value`` in every logit of the columns that do not count"""
    S = x.shape[2]
    dead = ~MR.mask(valid, S).to(x.device)
    return torch.where(dead[:, None, :], torch.full_like(x, value), x), dead


def forward(x, tg, rule, valid, entry="len"):
    """-> (probabilities, loss_part, correct_part); entry "ex": the unmasked call"""
    Bq, Q, S = x.shape
    guard = _Guard()
    y = guard.put(x, name="logits")
    parts = max(N.lib().mvn_ce_parts(Bq, S), 1)
    lp = guard.new((parts,), fill=0.0, name="loss_part")
    cp = guard.new((parts,), fill=0, name="correct_part", dtype=torch.int32)
    if entry == "ex":
        rc = N.lib().mvn_softmax_ce_forward_ex(y.data_ptr(), tg.data_ptr(), Bq, Q, S, lp.data_ptr(), cp.data_ptr(),
                                               rule, _stream())
    else:
        v = _dev_valid(valid)
        rc = N.lib().mvn_softmax_ce_forward_len(y.data_ptr(), tg.data_ptr(), Bq, Q, S, lp.data_ptr(), cp.data_ptr(),
                                                rule, None if v is None else v.data_ptr(), _stream())
    assert rc == N.MVN_OK, N.last_error()
    guard.check("softmax_ce forward")
    return y, lp, cp


def _window(S):
    col0, cols = 5, S + 37
    return col0, cols, col0 + cols + 22


def backward(p, tg, rule, valid, scale, entry="len"):
    Bq, Q, S = p.shape
    col0, cols, ld = _window(S)
    guard = _Guard()
    d = guard.new((Bq, Q, ld), fill=SENTINEL, name="dlogit")
    if entry == "ex":
        rc = N.lib().mvn_softmax_ce_backward_ex(p.data_ptr(), tg.data_ptr(), Bq, Q, S, scale, None, d.data_ptr(),
                                                Q * ld, ld, col0, cols, rule, _stream())
    else:
        v = _dev_valid(valid)
        rc = N.lib().mvn_softmax_ce_backward_len(p.data_ptr(), tg.data_ptr(), Bq, Q, S, scale, None, d.data_ptr(),
                                                 Q * ld, ld, col0, cols, rule, None if v is None else v.data_ptr(),
                                                 _stream())
    assert rc == N.MVN_OK, N.last_error()
    guard.check("softmax_ce backward")
    return d


@pytest.mark.parametrize("rule", sorted(RULES))
@pytest.mark.parametrize("Q,S", SHAPES)
def test_full_lengths_and_null_are_the_ex_calls_bit_for_bit(Q, S, rule):
    x, tg = _logits(Q, S, seed=Q + S)
    y0, lp0, cp0 = forward(x, tg, RULES[rule], None, entry="ex")
    d0 = backward(y0, tg, RULES[rule], None, 1.0 / (B * S), entry="ex")
    for valid in ([S] * B, None, [S + 1000] * B):
        y, lp, cp = forward(x, tg, RULES[rule], valid)
        assert torch.equal(_bits(y), _bits(y0)) and torch.equal(_bits(lp), _bits(lp0)) and torch.equal(cp, cp0), valid
        d = backward(y, tg, RULES[rule], valid, 1.0 / (B * S))
        assert torch.equal(_bits(d), _bits(d0)), valid


@pytest.mark.parametrize("rule", sorted(RULES))
@pytest.mark.parametrize("Q,S", SHAPES)
def test_masked_loss_and_gradient_vs_float64(Q, S, rule):
    x, tg = _logits(Q, S, seed=7 * Q + S)
    col0, cols, ld = _window(S)
    y_all, _, _ = forward(x, tg, RULES[rule], None, entry="ex")
    for valid in _valid_sets(S):
        vc = MR.clamp_valid(valid, S)
        y, lp, cp = forward(x, tg, RULES[rule], valid)
        assert torch.equal(_bits(y), _bits(y_all)), valid                  # every column's probabilities, as _ex
        loss, loss64 = lp.double().sum().item(), MR.masked_loss_sum(x, tg, valid, rule).item()
        print(f"Q {Q} S {S} {rule} valid {valid}: loss sum {loss:.6f} float64 {loss64:.6f} "
              f"rel {abs(loss - loss64) / max(loss64, 1e-300):.2e}")
        assert abs(loss - loss64) <= LOSS_TOL * loss64, valid
        assert int(cp.sum()) == MR.masked_correct(x, tg, valid), valid
        # the same input again: the same bits
        y2, lp2, cp2 = forward(x, tg, RULES[rule], valid)
        assert torch.equal(_bits(lp2), _bits(lp)) and torch.equal(cp2, cp) and torch.equal(_bits(y2), _bits(y))
        # NaN / +inf in the logits of the columns that do not count: loss and counts unchanged to the bit
        for value in (float("nan"), math.inf):
            xp, dead = _plant(x, valid, value)
            yp, lpp, cpp = forward(xp, tg, RULES[rule], valid)
            assert torch.equal(_bits(lpp), _bits(lp)) and torch.equal(cpp, cp), (valid, value)
            assert bool(torch.isfinite(lpp).all())
            assert torch.equal(_bits(yp)[~dead[:, None, :].expand_as(yp)], _bits(y)[~dead[:, None, :].expand_as(y)])
        scale = 1.0 / max(int(vc.sum()), 1)
        d = backward(y, tg, RULES[rule], valid, scale)
        want = MR.masked_dlogit(x, tg, valid, rule, scale)
        err = ((d[:, :, col0:col0 + S].cpu().double() - want).abs().max() / want.abs().max().clamp_min(1e-30)).item()
        print(f"  gradient err {err:.2e}")
        assert err < TOL, valid
        assert torch.equal(_bits(backward(y, tg, RULES[rule], valid, scale)), _bits(d))
        # probabilities that are NaN where nothing counts (what the forward leaves of planted NaN logits): the
        # window's masked columns are +0.0f exactly, the counted ones unchanged, nothing outside the window written
        xp, dead = _plant(x, valid, float("nan"))
        yp, _, _ = forward(xp, tg, RULES[rule], valid)
        assert bool(torch.isnan(yp).any()) == bool(dead.any())
        dp = backward(yp, tg, RULES[rule], valid, scale)
        assert torch.equal(_bits(dp), _bits(d)), valid
        for b in range(B):
            v = int(vc[b])
            assert bool((_bits(d[b, :, col0 + v:col0 + cols]) == 0).all()), (valid, b)     # +0.0f, not -0.0f
        assert bool((d[:, :, :col0] == SENTINEL).all()) and bool((d[:, :, col0 + cols:] == SENTINEL).all())


def _score(x, tg, valid, entry="len", want_entropy=True):
    Bq, Q, S = x.shape
    guard = _Guard()
    xin = guard.put(x, name="logits")
    out = {"logp": guard.new((Bq, S), fill=SENTINEL, name="logp"),
           "entropy": guard.new((Bq, S), fill=SENTINEL, name="entropy"),
           "rank": guard.new((Bq, S), fill=int(SENTINEL), name="rank", dtype=torch.int32),
           "seq_nll": guard.new((Bq,), fill=SENTINEL, name="seq_nll"),
           "seq_correct": guard.new((Bq,), fill=int(SENTINEL), name="seq_correct", dtype=torch.int32)}
    n = N.lib().mvn_score_scratch_floats(Bq, S)
    scratch = guard.new((max(n, 1),), fill=float("nan"), name="scratch")
    args = (xin.data_ptr(), tg.data_ptr(), Bq, Q, S, 1.0, out["logp"].data_ptr(),
            out["entropy"].data_ptr() if want_entropy else None, out["rank"].data_ptr(), out["seq_nll"].data_ptr(),
            out["seq_correct"].data_ptr(), scratch.data_ptr(), n)
    if entry == "plain":
        rc = N.lib().mvn_score_columns(*args, _stream())
    else:
        v = _dev_valid(valid)
        rc = N.lib().mvn_score_columns_len(*args, None if v is None else v.data_ptr(), _stream())
    assert rc == N.MVN_OK, N.last_error()
    guard.check("score_columns")
    assert torch.equal(_bits(xin), _bits(x))                               # read only
    return out


@pytest.mark.parametrize("Q,S", SHAPES)
def test_masked_score(Q, S):
    x, tg = _logits(Q, S, seed=13 * Q + S)
    for want_entropy in (True, False):
        plain = _score(x, tg, None, entry="plain", want_entropy=want_entropy)
        for valid in ([S] * B, None):
            got = _score(x, tg, valid, want_entropy=want_entropy)
            assert all(torch.equal(_bits(got[k]), _bits(plain[k])) for k in got), (valid, want_entropy)
    for valid in _valid_sets(S):
        got = _score(x, tg, valid)
        ref = MR.masked_score(x, tg, valid)
        keep = MR.mask(valid, S).to(DEV)
        for k in ("logp", "entropy"):
            err = ((got[k].cpu().double() - ref[k]).abs().max() / ref[k].abs().max().clamp_min(1e-300)).item()
            print(f"Q {Q} S {S} valid {valid}: {k} err {err:.2e}")
            assert err <= TOL, (valid, k)
        nll, nll64 = got["seq_nll"].cpu().double(), ref["seq_nll"]
        assert bool(((nll - nll64).abs() <= NLL_TOL * nll64.abs()).all()), valid
        assert torch.equal(got["rank"].cpu().long(), ref["rank"])
        assert torch.equal(got["seq_correct"].cpu().long(), ref["seq_correct"])
        assert all(torch.equal(_bits(v), _bits(got[k])) for k, v in _score(x, tg, valid).items())
        for value in (float("nan"), math.inf):
            xp, dead = _plant(x, valid, value)
            gp = _score(xp, tg, valid)
            assert all(torch.equal(_bits(gp[k]), _bits(got[k])) for k in got), (valid, value)
        assert bool((_bits(got["logp"])[~keep] == 0).all()) and bool((_bits(got["entropy"])[~keep] == 0).all())
        assert bool((got["rank"][~keep] == -1).all())
