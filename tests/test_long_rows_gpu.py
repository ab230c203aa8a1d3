"""GPU: the full-sequence path on rows whose (Q, ld) tensors reach past a 32-bit byte offset.

Several kernels address one sequence's rows through a raw buffer resource with 32-bit offsets (the column softmax /
loss kernels, the head's strip kernels): row q, column t at byte 4 (q ld + t).  A small C = K = 64 stack (short
receptive field, little memory) runs at three lengths per class count Q (tests/helpers.py long_row_lengths): just
below the limit, with only the last row's tail past it, and with the top ~15 % of the rows past it.

The model is causal, so columns [c0, c0 + W) of the output equal the float64 oracle run on inputs [c0 - 1, c0 + W +
RF - 1) alone: windows at the start, in the middle, at the first column past the limit and at the end are compared
with it, all Q rows.  Gradients of sum(out * mask), mask nonzero on those windows only, are the sum of the windows'
own gradients."""
import pytest
import torch
import torch.nn.functional as F

from helpers import OFFSET_LIMIT, long_row_lengths, rel_err
from movenet_amd import _native as N
from movenet_amd.utils.weights import make_state_dict
from oracle import wavenet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W = 2048


def _cfg(Q):
    return dict(layer_size=2, stack_size=1, input_channels=Q, residual_channels=64, skip_channels=64)


def _model(cfg, sd):
    from movenet_amd.wavenet import WaveNet
    m = WaveNet(**cfg)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


def _t_len(Q, where, rf):
    """t_len whose head tensors (B, Q, Sp) have row stride long_row_lengths(Q)[where]; the output's stride is 64 less"""
    ld = long_row_lengths(Q)[where]
    S = ld - 64                                    # Sp = pad64(S + 31) = ld
    assert N.lib().mvn_padded_len(S + 31) == ld
    return S + rf - 1


def _first_bad_col(Q, ld):
    """output column of the first element of a (Q, ld) tensor at or past the limit (None when none is)"""
    q = (OFFSET_LIMIT // 4) // ld
    if q >= Q:
        return None
    return (OFFSET_LIMIT // 4) - q * ld


def _windows(Q, S_out, Sp, pad):
    starts = [0, S_out // 2]
    for ld, shift in ((S_out, 0), (Sp, -pad)):   # (head column c of the Sp-strided tensors = output column c - pad)
        c = _first_bad_col(Q, ld)
        if c is not None:
            starts.append(max(0, min(S_out - W, c + shift - W // 2)))
    starts.append(S_out - W)
    out = []
    for c0 in sorted(starts):  # non-overlapping, in order
        if out and c0 < out[-1] + W:
            c0 = out[-1] + W
        if c0 + W <= S_out:
            out.append(c0)
    return out


def _oracle_window(sd64, dims, x_idx, c0, rf, normalized):
    """float64 oracle on one window's receptive field: output columns [c0, c0 + W) of (B, Q, W)"""
    lo = max(0, c0 - 1)
    idx = x_idx[:, lo:c0 + W + rf - 1].cpu()
    x = F.one_hot(idx, dims.input_channels).permute(0, 2, 1).double()
    out = O.forward(sd64, dims, x, output_unnormalized=normalized, remove_last=False)
    return out[:, :, -W:]


def _one_hot(idx, Q):
    x = torch.zeros(idx.shape[0], Q, idx.shape[1], device=DEV)
    x.scatter_(1, idx[:, None, :].long(), 1.0)
    return x


CASES = [(256, w) for w in ("below", "tail", "past")] + [(128, w) for w in ("below", "tail", "past")]


# MOVENET_HIP_FORWARD_MFMA=f32: the fp32 dense strip of the Q = 256 head (Q = 128 has no such form)
@pytest.mark.parametrize("Q,where,mfma", [c + ("default",) for c in CASES] + [(256, w, "f32") for w in ("below", "tail", "past")])
def test_long_row_forward_windows_vs_float64(Q, where, mfma, monkeypatch):
    if mfma == "f32":
        monkeypatch.setenv("MOVENET_HIP_FORWARD_MFMA", "f32")  # (read again by the next forward: MOVENET_DEBUG_GUARD)
    cfg = _cfg(Q)
    dims = O.Dims(**cfg)
    rf = dims.receptive_fields
    T = _t_len(Q, where, rf)
    sd = make_state_dict(**cfg, seed=21, gain=1.5)
    sd64 = {k: v.double() for k, v in sd.items()}
    m = _model(cfg, sd).eval()
    worst = {}
    for B in (1, 2):
        g = torch.Generator(device=DEV).manual_seed(5 + B)
        idx = torch.randint(0, Q, (B, T), generator=g, device=DEV)
        x = _one_hot(idx, Q)
        for normalized in (True, False):
            with torch.no_grad():
                out = m(x, output_unnormalized=normalized)
            S_out = out.shape[2]
            Sp = N.lib().mvn_padded_len(S_out + 1 + 31)
            assert bool(torch.isfinite(out).all())
            if normalized:
                assert (out.sum(1, dtype=torch.float64) - 1).abs().max().item() < 1e-5
            for c0 in _windows(Q, S_out, Sp, (rf - 1) & 31):
                want = _oracle_window(sd64, dims, idx, c0, rf, normalized)
                e = rel_err(out[:, :, c0:c0 + W].cpu(), want)
                worst[(B, normalized, c0)] = e
            del out
        del x
        torch.cuda.empty_cache()
    bad = {k: v for k, v in worst.items() if not v < 2e-5}
    assert not bad, (Q, where, mfma, bad)


@pytest.mark.parametrize("Q,where", CASES)
def test_long_row_backward_windows_vs_float64(Q, where):
    cfg = _cfg(Q)
    dims = O.Dims(**cfg)
    rf = dims.receptive_fields
    T = _t_len(Q, where, rf)
    Tp = N.lib().mvn_padded_len(T)
    sd = make_state_dict(**cfg, seed=22, gain=1.5)
    m = _model(cfg, sd).train()
    g = torch.Generator(device=DEV).manual_seed(9)
    idx = torch.randint(0, Q, (1, T), generator=g, device=DEV)
    x = _one_hot(idx, Q)
    out = m(x)
    S_out = out.shape[2]
    Sp = N.lib().mvn_padded_len(S_out + 1 + 31)
    wins = _windows(Q, S_out, Sp, (rf - 1) & 31)
    mask = torch.zeros_like(out)
    gm = torch.Generator().manual_seed(3)
    masks = []
    for c0 in wins:
        mw = torch.randn(1, Q, W, generator=gm, dtype=torch.float64)
        masks.append(mw)
        mask[:, :, c0:c0 + W] = mw.float().to(DEV)
    (out * mask).sum().backward()
    form = N.lib().mvn_last_backward_form()
    del out, mask
    torch.cuda.empty_cache()
    params = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    for c0, mw in zip(wins, masks):
        want = _oracle_window(params, dims, idx, c0, rf, True)
        (want * mw.float().double()).sum().backward()
    errs = {}
    for k, p in m.named_parameters():
        go = params[k].grad
        if go is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
        else:
            errs[k] = rel_err(p.grad.cpu(), go)
    bad = {k: v for k, v in errs.items() if not v < 3e-4}
    assert not bad, (Q, where, form, bad)
    if Tp > (1 << 21):
        # the one-kernel layer backward's buffers span 2^21 columns: the split halves run while their (2C, Tp) dfg
        # tensor fits a buffer resource, the generic form beyond
        assert form == (N.BWD_FORM_HALVES if 4 * 128 * Tp <= 0x7FFFFFFF else N.BWD_FORM_GENERIC), form
        # and the bf16 layer kernels refuse the length instead of computing it
        m.forward_precision = "bf16"
        with pytest.raises(ValueError):
            m(x)
    del x
    torch.cuda.empty_cache()


def test_fused_loss_past_the_limit_vs_float64():
    """one trainer step (wavenet_forward_loss) at Q = 256 with the top rows past the limit: loss and accuracy over
    every column against a float64 double-softmax cross entropy of the kernel's own logits, and the head's gradients
    against the float64 oracle run block by block over the whole sequence"""
    from movenet_amd.ops import wavenet_forward_loss
    Q = 256
    cfg = _cfg(Q)
    dims = O.Dims(**cfg)
    rf = dims.receptive_fields
    T = _t_len(Q, "past", rf)
    sd = make_state_dict(**cfg, seed=23, gain=1.5)
    m = _model(cfg, sd).train()
    g = torch.Generator(device=DEV).manual_seed(11)
    idx = torch.randint(0, Q, (1, T), generator=g, device=DEV)
    x = _one_hot(idx, Q)
    with torch.no_grad():
        logits = m(x, output_unnormalized=False)
    S = logits.shape[2]
    tg = idx[:, rf:]
    assert tg.shape == (1, S)
    loss64, step = 0.0, 1 << 18
    for c0 in range(0, S, step):
        p = torch.softmax(logits[:, :, c0:c0 + step].double(), 1)
        loss64 += (torch.logsumexp(p, 1) - p.gather(1, tg[:, None, c0:c0 + step]).squeeze(1)).sum().item()
    loss64 /= S
    del logits
    torch.cuda.empty_cache()
    loss, acc, probs = wavenet_forward_loss(m, x)
    # (the loss: fp32 sums of 64 columns, then torch's fp32 tree sum of ~S / 64 of them: error ~ log2(S) eps)
    assert abs(loss.item() - loss64) < 1e-5 * loss64, (loss.item(), loss64)
    count = int((probs.argmax(1) == tg).sum())
    assert acc.item() == torch.tensor(count, dtype=torch.float32, device=DEV).div(S).item()
    del probs
    loss.backward()
    del x
    torch.cuda.empty_cache()
    # float64 oracle block by block: output block [c0, c1) needs inputs [c0 - 1, c1 + rf - 1)
    params = {k: v.double().to(DEV).requires_grad_(True) for k, v in sd.items()}
    for c0 in range(0, S, step):
        c1 = min(S, c0 + step)
        lo = max(0, c0 - 1)
        xs = F.one_hot(idx[:, lo:c1 + rf - 1].long(), Q).permute(0, 2, 1).double()
        p = O.forward(params, dims, xs, remove_last=False)[:, :, -(c1 - c0):]
        F.cross_entropy(p, tg[:, c0:c1], reduction="sum").div(S).backward()
        del xs, p
    # Every column carries loss here, so each weight gradient is a sum of S ~ 2.5 M signed fp32 terms (512-column
    # partial sums, then a sum of the partials).  Its rounding error grows like sqrt(S) for terms of random sign: the
    # suite's 3e-4 holds at the config-2 length of 16 000 columns, so the bound is 3e-4 sqrt(S / 16000) (~3.7e-3).  A
    # dropped row or column moves these gradients by 0.5 - 20 (relative).
    tol = 3e-4 * (S / 16000) ** 0.5
    for k in ("dense_conv.conv2.weight", "dense_conv.conv2.bias", "dense_conv.conv1.weight", "dense_conv.conv1.bias"):
        e = rel_err(dict(m.named_parameters())[k].grad.cpu(), params[k].grad.cpu())
        assert e < tol, (k, e, tol)
    torch.cuda.empty_cache()
