"""GPU: the trainer's loss kernels through the C ABI, at the edges of their dispatch, against float64 torch.

``mvn_softmax_ce_forward`` / ``_backward`` (softmax + cross_entropy ON the probabilities + accuracy, and its gradient
into a padded dlogit window) and ``mvn_ce_on_probs_forward`` / ``_backward``, called the way movenet_amd.ops calls
them, on synthetic logits: the column forms (Q <= 256, padding rows for Q not a multiple of 64) against the
one-thread-per-column forms (Q > 256) on the same data, column counts that are not a multiple of 64 or 256, exact
ties in the argmax, logits spread past sm_exp's underflow cut, the dlogit window's zeroed and untouched columns,
the upstream gradient, and rows past the 32-bit offset limit of one sequence's (Q, S) tensor."""
import numpy as np
import pytest
import torch

from helpers import first_bad_row, long_row_lengths
from movenet_amd import _native as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -1234.5
# elementwise fp32 outputs (probabilities, gradients) against float64: max |err| / max |ref|, the logits bound of
# test_reference_shapes_gpu.py
TOL = 2e-5


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


def _ref_softmax_ce(x, tg):
    """float64: probabilities, per-column loss of cross_entropy(probs) and d loss / d logits with scale 1."""
    x = x.double()
    p = torch.softmax(x, 1)
    lse = torch.logsumexp(p, 1)
    pt = p.gather(1, tg[:, None]).squeeze(1)
    loss = lse - pt
    g = torch.softmax(p, 1)
    g.scatter_add_(1, tg[:, None], -torch.ones_like(pt)[:, None])
    dlogit = p * (g - (g * p).sum(1, keepdim=True))
    return p, loss, dlogit


def _ref_ce_on_probs(p, tg):
    p = p.double()
    lse = torch.logsumexp(p, 1)
    loss = lse - p.gather(1, tg[:, None]).squeeze(1)
    g = torch.softmax(p, 1)
    g.scatter_add_(1, tg[:, None], -torch.ones_like(loss)[:, None])
    return loss, g


def _err(got, want):
    return ((got.double() - want).abs().max() / want.abs().max().clamp_min(1e-30)).item()


def _correct(p, tg):
    """first-maximum argmax of the kernel's own fp32 probabilities (torch.argmax's rule), on the host"""
    return int((p.cpu().argmax(1) == tg.cpu()).sum())


def softmax_ce_forward(x, tg):
    lib = N.lib()
    B, Q, S = x.shape
    y = x.clone()
    parts = max(lib.mvn_ce_parts(B, S), 1)
    lp = torch.zeros(parts, dtype=torch.float32, device=DEV)
    cp = torch.zeros(parts, dtype=torch.int32, device=DEV)
    N.check(lib.mvn_softmax_ce_forward(y.data_ptr(), tg.data_ptr(), B, Q, S, lp.data_ptr(), cp.data_ptr(), _stream()),
            "mvn_softmax_ce_forward")
    return y, lp.double().sum().item(), int(cp.sum())


def softmax_ce_backward(p, tg, scale, upstream, ld, col0, cols):
    lib = N.lib()
    B, Q, S = p.shape
    d = torch.full((B, Q, ld), SENTINEL, dtype=torch.float32, device=DEV)
    N.check(lib.mvn_softmax_ce_backward(p.data_ptr(), tg.data_ptr(), B, Q, S, scale,
                                        None if upstream is None else upstream.data_ptr(), d.data_ptr(), Q * ld, ld,
                                        col0, cols, _stream()), "mvn_softmax_ce_backward")
    return d


def ce_on_probs(p, tg, scale, upstream):
    lib = N.lib()
    B, Q, S = p.shape
    parts = max(lib.mvn_ce_parts(B, S), 1)
    lp = torch.zeros(parts, dtype=torch.float32, device=DEV)
    cp = torch.zeros(parts, dtype=torch.int32, device=DEV)
    N.check(lib.mvn_ce_on_probs_forward(p.data_ptr(), tg.data_ptr(), B, Q, S, lp.data_ptr(), cp.data_ptr(), _stream()),
            "mvn_ce_on_probs_forward")
    dp = torch.full_like(p, SENTINEL)
    N.check(lib.mvn_ce_on_probs_backward(p.data_ptr(), tg.data_ptr(), B, Q, S, scale,
                                         None if upstream is None else upstream.data_ptr(), dp.data_ptr(), _stream()),
            "mvn_ce_on_probs_backward")
    return lp.double().sum().item(), int(cp.sum()), dp


# Q: 2, 100 and 200 (column forms with padding rows), 256 (column form, no padding), 257 and 300 (one thread per
# column); S: 1, not a multiple of 64, not a multiple of 256
@pytest.mark.parametrize("Q", [2, 100, 200, 256, 257, 300])
@pytest.mark.parametrize("S", [1, 333, 700])
def test_softmax_ce_forward_and_backward_vs_float64(Q, S):
    B = 2
    x, tg = _logits(B, Q, S, seed=Q * 1000 + S)
    y, loss, correct = softmax_ce_forward(x, tg)
    p64, loss64, dlogit64 = _ref_softmax_ce(x, tg)
    assert _err(y, p64) < TOL
    assert abs(loss - loss64.sum().item()) < 1e-5 * loss64.sum().item()
    assert correct == _correct(y, tg)
    # backward into a padded window: columns [col0, col0 + cols) of rows of ld, cols > S (the extra ones zeroed),
    # everything outside the window untouched; scale and upstream multiply
    col0, cols = 5, S + 37
    ld = col0 + cols + 22
    scale, up = 1.0 / (B * S), torch.tensor([2.5], device=DEV)
    for upstream, factor in ((None, scale), (up, 2.5 * scale)):
        d = softmax_ce_backward(y, tg, scale, upstream, ld, col0, cols)
        want = _ref_grad_from_probs(y, tg)  # (the gradient at the kernel's OWN probabilities)
        assert _err(d[:, :, col0:col0 + S], factor * want) < TOL, upstream
        assert bool((d[:, :, col0 + S:col0 + cols] == 0).all())
        assert bool((d[:, :, :col0] == SENTINEL).all()) and bool((d[:, :, col0 + cols:] == SENTINEL).all())
    # the loss forward's gradient matches the float64 gradient through the logits as well
    d = softmax_ce_backward(y, tg, 1.0, None, S, 0, S)
    assert _err(d, dlogit64) < TOL


def _ref_grad_from_probs(p, tg):
    """float64 d loss / d logits given the (fp32) probabilities the forward wrote: what the backward kernel reads"""
    p = p.double()
    g = torch.softmax(p, 1)
    g.scatter_add_(1, tg[:, None], -torch.ones(g.shape[0], 1, g.shape[2], dtype=g.dtype, device=g.device))
    return p * (g - (g * p).sum(1, keepdim=True))


@pytest.mark.parametrize("Q", [2, 100, 256, 257])
@pytest.mark.parametrize("S", [1, 333])
def test_ce_on_probs_vs_float64(Q, S):
    B = 3
    # inputs are taken as they come (the model's probabilities in the trainer, anything here): spread wide enough that
    # sm_exp's x < -103 cut is taken
    p, tg = _logits(B, Q, S, seed=7 + Q + S, spread=60.0)
    loss64, g64 = _ref_ce_on_probs(p, tg)
    for upstream, factor in ((None, 0.5), (torch.tensor([3.0], device=DEV), 1.5)):
        loss, correct, dp = ce_on_probs(p, tg, 0.5, upstream)
        assert abs(loss - loss64.sum().item()) < 1e-5 * loss64.abs().sum().item()
        assert correct == _correct(p, tg)
        assert _err(dp, factor * g64) < TOL


@pytest.mark.parametrize("Q", [2, 100, 256, 257])
def test_argmax_ties_take_the_first_maximum(Q):
    """exact ties: the accuracy counts a column only when the target is the FIRST maximal class"""
    B, S = 2, 333
    x, tg = _logits(B, Q, S, seed=99 + Q, ties=True)
    y, _, correct = softmax_ce_forward(x, tg)
    want = _correct(y, tg)
    assert correct == want
    ties = (y == y.amax(1, keepdim=True)).sum(1) > 1
    assert int(ties.sum()) >= B * (S // 3)  # the probabilities of tied logits tie exactly
    _, correct2, _ = ce_on_probs(x, tg, 1.0, None)
    assert correct2 == _correct(x, tg)
    # moving the target to the first tied class makes those columns count
    tg2 = tg.clone()
    tg2[:, ::3] = x[:, :, ::3].cpu().argmax(1).to(DEV)
    _, _, c3 = softmax_ce_forward(x, tg2)
    assert c3 == _correct(y, tg2) and c3 >= B * len(range(0, S, 3))


@pytest.mark.parametrize("Q", [256, 257])
def test_exp_underflow_spread(Q):
    """logits 200 apart: most exponentials of the first softmax are below sm_exp's cut and exactly 0"""
    B, S = 2, 200
    x, tg = _logits(B, Q, S, seed=5, spread=100.0)
    y, loss, correct = softmax_ce_forward(x, tg)
    p64, loss64, _ = _ref_softmax_ce(x, tg)
    assert bool((y == 0).any()) and bool(torch.isfinite(y).all())
    assert _err(y, p64) < TOL
    assert abs(loss - loss64.sum().item()) < 1e-5 * loss64.sum().item()
    assert correct == _correct(y, tg)
    d = softmax_ce_backward(y, tg, 1.0, None, S, 0, S)
    assert bool(torch.isfinite(d).all()) and _err(d, _ref_grad_from_probs(y, tg)) < TOL


def _chunked_checks(x, y, tg, d, Q, S):
    """float64 references column block by column block (a whole (256, 2.4 M) float64 tensor is 5 GB)"""
    worst_p = worst_d = 0.0
    loss64 = 0.0
    step = 1 << 18
    for c0 in range(0, S, step):
        c1 = min(S, c0 + step)
        p64, l64, _ = _ref_softmax_ce(x[:, :, c0:c1], tg[:, c0:c1])
        worst_p = max(worst_p, _err(y[:, :, c0:c1], p64))
        loss64 += l64.sum().item()
        if d is not None:
            worst_d = max(worst_d, _err(d[:, :, c0:c1], _ref_grad_from_probs(y[:, :, c0:c1], tg[:, c0:c1])))
        del p64, l64
    return worst_p, worst_d, loss64


@pytest.mark.parametrize("where", ["below", "tail", "past"])
def test_column_forms_past_the_offset_limit(where):
    """one sequence of Q = 256 rows whose length puts the last rows' offsets at or past 2^31 bytes: every row of the
    probabilities, the loss, the accuracy and the gradient must still be right"""
    Q = 256
    S = long_row_lengths(Q)[where]
    B = 1
    g = torch.Generator(device=DEV).manual_seed(17)
    x = torch.randn(B, Q, S, generator=g, device=DEV) * 4.0
    tg = torch.randint(0, Q, (B, S), generator=g, device=DEV)
    y, loss, correct = softmax_ce_forward(x, tg)
    d = torch.empty_like(y)
    N.check(N.lib().mvn_softmax_ce_backward(y.data_ptr(), tg.data_ptr(), B, Q, S, 1.0, None, d.data_ptr(), Q * S, S,
                                            0, S, _stream()), "mvn_softmax_ce_backward")
    # the last row, where an offset past the limit shows first: its tail columns must not have been dropped
    assert bool((y[0, Q - 1, -64:] > 0).all()) and bool((d[0, Q - 1, -64:] != 0).any())
    worst_p, worst_d, loss64 = _chunked_checks(x, y, tg, d, Q, S)
    bad = first_bad_row(Q, S)
    assert worst_p < TOL, (where, bad, worst_p)
    assert worst_d < TOL, (where, bad, worst_d)
    # (the loss: fp32 sums of 64 columns, added in float64 here: the bound does not grow with S)
    assert abs(loss - loss64) < 1e-5 * loss64, (loss, loss64)
    assert correct == _correct(y, tg)
    # the probabilities of each column sum to 1 (fp32 terms, Q of them)
    assert (y.sum(1, dtype=torch.float64) - 1).abs().max().item() < 1e-5
    # ce_on_probs on the same rows (dprobs goes to a second (Q, S) tensor)
    del d
    lossb, correctb, dp = ce_on_probs(y, tg, 1.0, None)
    step = 1 << 18
    worst, l64 = 0.0, 0.0
    for c0 in range(0, S, step):
        c1 = min(S, c0 + step)
        lo, gr = _ref_ce_on_probs(y[:, :, c0:c1], tg[:, c0:c1])
        worst = max(worst, _err(dp[:, :, c0:c1], gr))
        l64 += lo.sum().item()
    assert worst < TOL, (where, bad, worst)
    assert abs(lossb - l64) < 1e-5 * l64 and correctb == correct
    del x, y, dp
    torch.cuda.empty_cache()
