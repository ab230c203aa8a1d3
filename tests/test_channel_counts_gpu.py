"""GPU: class counts Q and channel counts C / K that no other test runs, against the float64 oracle.

Each row of the table reaches a branch of the full-sequence path's dispatch: Q = 2, 100, 200 (the column softmax and
loss kernels with padding rows, the generic head), Q = 257, 512 (the one-thread-per-column softmax and loss kernels),
all with the fused C = K = 64 layer kernels; and (C, K) = (64, 32), (32, 64), (24, 40), (1, 1), (256, 256) at Q = 256
(the generic layer forms, C != K, channel counts that are not a multiple of 16).  Per row: logits, probabilities,
the model path's loss and every parameter gradient against torch autograd on the oracle in float64; the fused loss
node against the unfused one; greedy generation through whatever mvn_gen_variant(AUTO) picks."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import one_hot, rel_err, synthetic_indices
from movenet_amd import _native as N
from movenet_amd.utils.weights import make_state_dict
from oracle import wavenet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOGIT_TOL, GRAD_TOL = 2e-5, 3e-4  # test_reference_shapes_gpu.py

ROWS = [(Q, 64, 64) for Q in (2, 100, 200, 257, 512)] + [(256, C, K) for C, K in ((64, 32), (32, 64), (24, 40), (1, 1),
                                                                                     (256, 256))]


def _cfg(Q, C, K):
    return dict(layer_size=2, stack_size=2, input_channels=Q, residual_channels=C, skip_channels=K)


def _model(cfg, sd):
    from movenet_amd.wavenet import WaveNet
    m = WaveNet(**cfg)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


@pytest.mark.parametrize("Q,C,K", ROWS)
def test_forward_loss_gradients_vs_float64(Q, C, K):
    from movenet_amd.ops import cross_entropy_on_probs, wavenet_forward_loss
    cfg = _cfg(Q, C, K)
    dims = O.Dims(**cfg)
    rf = dims.receptive_fields
    B, T = 3, rf + 300
    sd = make_state_dict(**cfg, seed=31, gain=1.5)
    x = one_hot(synthetic_indices(B, T, Q, 77), Q)
    target = x[:, :, rf:].argmax(1)
    params = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    logits_o = O.forward(params, dims, x.double(), output_unnormalized=False)
    probs_o = O.forward(params, dims, x.double())
    loss_o = F.cross_entropy(probs_o, target)
    loss_o.backward()
    m = _model(cfg, sd).train()
    xd = x.to(DEV)
    with torch.no_grad():
        logits = m(xd, output_unnormalized=False)
    assert logits.shape == logits_o.shape
    assert rel_err(logits.cpu(), logits_o.detach()) < LOGIT_TOL
    probs = m(xd)
    assert rel_err(probs.detach().cpu(), probs_o.detach()) < LOGIT_TOL
    loss = F.cross_entropy(probs, target.to(DEV))
    loss.backward()
    assert abs(loss.item() - loss_o.item()) < 2e-6 * max(1.0, abs(loss_o.item()))
    for k, p in m.named_parameters():
        go = params[k].grad
        if go is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
        else:
            assert rel_err(p.grad.cpu(), go) < GRAD_TOL, k
    # the fused loss node: the same bits as the plain forward + cross_entropy_on_probs, the same gradients
    m.zero_grad(set_to_none=True)
    out = m(xd)
    loss1, acc1 = cross_entropy_on_probs(out, target.to(DEV))
    loss1.backward()
    want = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    loss2, acc2, probs2 = wavenet_forward_loss(m, xd)
    assert torch.equal(probs2, out.detach())
    assert loss2.item() == loss1.item() and acc2.item() == acc1.item()
    assert abs(loss2.item() - loss_o.item()) < 2e-6 * max(1.0, abs(loss_o.item()))
    assert acc2.item() == (probs2.argmax(1) == target.to(DEV)).float().mean().item()
    (2.0 * loss2).backward()
    got = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    assert sorted(got) == sorted(want)
    # (the two nodes round dlogit differently by an ulp: the bound is 2e-6, or -- for a gradient that is a cancelling sum,
    # C = 1's biases -- twice the unfused gradient's own deviation from float64, whichever is larger)
    for k in want:
        w = 2.0 * want[k].cpu()
        own = rel_err(w, 2.0 * params[k].grad)
        assert rel_err(got[k].cpu(), 2.0 * params[k].grad) < GRAD_TOL, k
        assert rel_err(got[k].cpu(), w) < max(2e-6, 2.0 * own), (k, own)


@pytest.mark.parametrize("Q,C,K", ROWS)
def test_greedy_generation_vs_float64(Q, C, K):
    """AUTO takes the generic generator for every row (the STREAM / PIPE / FOLD kernels need C = K = 64 and Q in
    {64, 128, 256}); its teacher-forced logits against the float64 oracle over the same sequence, and its free-run
    picks wherever the top-2 margin clears the tolerance"""
    from movenet_amd.generation import RingGenerator
    cfg = _cfg(Q, C, K)
    dims = O.Dims(**cfg)
    rf = dims.receptive_fields
    B, n_new = 3, 40
    picked = N.lib().mvn_gen_variant(N.make_dims(2, 2, Q, C, K), N.GEN_AUTO, B)
    assert picked == N.GEN_GENERIC, picked
    sd = make_state_dict(**cfg, seed=1, gain=2.0, head_gain=6.0)
    prompt = synthetic_indices(B, rf, Q, 4321)
    gen = RingGenerator(**cfg, state_dict={k: v.to(DEV) for k, v in sd.items()}, batch=B, n_total=rf + n_new, device=DEV,
                        variant=N.GEN_AUTO, temperature=0.0)
    assert gen.variant == N.GEN_GENERIC
    gen.prime(prompt.to(DEV))
    gen.advance(n_new)
    gen.check_errors()
    seq = gen.samples.clone()
    assert torch.equal(seq[:, :rf].cpu(), prompt.to(seq.dtype))
    _, logits = gen.teacher_forced(seq, logits_t0=rf)
    gen.check_errors()
    # oracle column s = the logits after consuming time s + rf - 1, which pick time s + rf
    x = F.one_hot(seq.cpu().long(), Q).permute(0, 2, 1).double()
    want = O.forward({k: v.double() for k, v in sd.items()}, dims, x, output_unnormalized=False,
                     remove_last=False)[:, :, :n_new].permute(0, 2, 1).numpy()
    got = logits.cpu().numpy()
    assert got.shape == want.shape == (B, n_new, Q)
    assert rel_err(got, want) < LOGIT_TOL
    top2 = np.sort(want, axis=2)[:, :, -2:]
    clear = (top2[:, :, 1] - top2[:, :, 0]) > 4 * LOGIT_TOL * np.abs(want).max()
    assert clear.mean() > 0.5
    picks = seq[:, rf:].cpu().numpy()
    assert np.array_equal(picks[clear], want.argmax(2)[clear])
