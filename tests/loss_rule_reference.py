"""Float64 restatement of the "model" loss rule (include/movenet_hip.h, MVN_LOSS_MODEL): the negative log-likelihood
of softmax(logits) and its gradient with respect to the logits.  Torch only, written out from the definition (no
cross_entropy, no autograd); shared by the loss-rule tests, which hold it to torch's own on the CPU."""
from __future__ import annotations

import torch


def clamp_target(target: torch.Tensor, classes: int) -> torch.Tensor:
    """The kernels' rule for a target outside [0, Q - 1]: the nearest class."""
    return target.to(torch.int64).clamp(0, classes - 1)


def model_probs(logits: torch.Tensor) -> torch.Tensor:
    """softmax over dim 1 of (B, Q, S) logits, in float64, the maximum subtracted first."""
    x = logits.double()
    e = torch.exp(x - x.amax(1, keepdim=True))
    return e / e.sum(1, keepdim=True)


def model_loss_columns(logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """(B, S) float64: logsumexp_q(logits[b, :, s]) - logits[b, target[b, s], s], i.e. -log p_target in nats."""
    x = logits.double()
    m = x.amax(1)
    lse = m + torch.log(torch.exp(x - m[:, None]).sum(1))
    tg = clamp_target(target, x.shape[1])
    return lse - x.gather(1, tg[:, None]).squeeze(1)


def onehot(target: torch.Tensor, classes: int) -> torch.Tensor:
    """(B, Q, S) float64 indicator of the (clamped) target class."""
    tg = clamp_target(target, classes)
    out = torch.zeros(tg.shape[0], classes, tg.shape[1], dtype=torch.float64, device=tg.device)
    return out.scatter_(1, tg[:, None], 1.0)


def model_dlogit(probs: torch.Tensor, target: torch.Tensor, factor: float = 1.0) -> torch.Tensor:
    """factor (p - onehot(target)) in float64: d (factor sum of the columns' losses) / d logits, given the
    probabilities (the kernel's own fp32 ones, or ``model_probs`` of the logits)."""
    p = probs.double()
    return factor * (p - onehot(target, p.shape[1]))
