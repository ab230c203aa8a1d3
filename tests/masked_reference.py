"""Float64 restatement of the loss and the score over sequences of their own length (include/movenet_hip.h, the _len
entry points): sequence b counts its columns s < valid_b, valid_b = clamp(len_b - RF, 0, S); loss and accuracy are
sums over those columns divided by max(N_valid, 1); d loss / d logits is 0 on every other column.  Torch on the CPU
only; the gradient is torch autograd's."""
from __future__ import annotations

import torch

import score_reference as SR

RULES = ("reference", "model")


def clamp_valid(valid, S: int) -> torch.Tensor:
    """(B,) int64: the kernels' clamp of the per-sequence column counts to [0, S]."""
    return torch.as_tensor(valid, dtype=torch.int64).clamp(0, S)


def valid_columns(lengths, T: int, RF: int) -> list:
    """The definition: valid_b = clamp(len_b - RF, 0, T - RF)."""
    return [min(max(int(n) - RF, 0), T - RF) for n in lengths]


def mask(valid, S: int) -> torch.Tensor:
    """(B, S) bool: column s of sequence b counts."""
    return torch.arange(S)[None, :] < clamp_valid(valid, S)[:, None]


def column_losses(logits: torch.Tensor, target: torch.Tensor, rule: str) -> torch.Tensor:
    """(B, S) float64 loss of every column: "model" -log softmax(logits)[target]; "reference" cross_entropy applied
    to the PROBABILITIES, -log softmax(softmax(logits))[target]."""
    x = logits.double()
    tg = target.to(torch.int64).clamp(0, x.shape[1] - 1)
    if rule == "reference":
        x = torch.softmax(x, dim=1)
    else:
        assert rule == "model", rule
    return -torch.log_softmax(x, dim=1).gather(1, tg[:, None]).squeeze(1)


def masked_loss_sum(logits, target, valid, rule: str) -> torch.Tensor:
    """float64 scalar: the sum of the counted columns' losses (what loss_part adds up to)."""
    S = logits.shape[2]
    return torch.where(mask(valid, S), column_losses(logits.cpu(), target.cpu(), rule), torch.zeros((), dtype=torch.float64)).sum()


def masked_correct(logits, target, valid) -> int:
    """number of counted columns whose (clamped) target is the first maximum of the probabilities"""
    x = logits.cpu().double()
    tg = target.cpu().to(torch.int64).clamp(0, x.shape[1] - 1)
    return int(((torch.softmax(x, 1).argmax(1) == tg) & mask(valid, x.shape[2])).sum())


def masked_loss(logits, target, valid, rule: str):
    """(loss, accuracy) as floats: sums over the counted columns / max(N_valid, 1)."""
    n = max(int(clamp_valid(valid, logits.shape[2]).sum()), 1)
    return masked_loss_sum(logits, target, valid, rule).item() / n, masked_correct(logits, target, valid) / n


def masked_dlogit(logits, target, valid, rule: str, factor: float) -> torch.Tensor:
    """(B, Q, S) float64: d (factor * masked_loss_sum) / d logits by autograd.  The logits of the columns that do not
    count never enter the sum, so they are replaced by zeros first (they may hold NaN) and their gradient is 0."""
    S = logits.shape[2]
    keep = mask(valid, S)[:, None, :]
    x = torch.where(keep, logits.cpu().double(), torch.zeros((), dtype=torch.float64)).requires_grad_(True)
    (factor * masked_loss_sum(x, target.cpu(), valid, rule)).backward()
    return torch.where(keep, x.grad, torch.zeros((), dtype=torch.float64))


def masked_score(logits, target, valid, temperature: float = 1.0) -> dict:
    """score_reference.score with the columns that do not count taken out: logp = entropy = 0, rank = -1 there, and
    seq_nll / seq_correct over the counted columns only (float64 / int64, on the CPU)."""
    S = logits.shape[2]
    keep = mask(valid, S)
    x = torch.where(keep[:, None, :], logits.cpu().double(), torch.zeros((), dtype=torch.float64))
    ref = SR.score(x, target.cpu(), temperature)
    logp = torch.where(keep, ref["logp"], torch.zeros((), dtype=torch.float64))
    rank = torch.where(keep, ref["rank"], torch.full((), -1, dtype=ref["rank"].dtype))
    return {"logp": logp, "entropy": torch.where(keep, ref["entropy"], torch.zeros((), dtype=torch.float64)),
            "rank": rank, "seq_nll": -logp.sum(1), "seq_correct": (rank == 0).sum(1)}
