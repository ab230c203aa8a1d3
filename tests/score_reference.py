"""Float64 restatement of mvn_score_columns (not a test): the five outputs from fp32 logits, target clamp and tie rule
included.  With y = logits / temperature, all in float64:

    logp[b,s]      = y_t - logsumexp_q(y)
    entropy[b,s]   = -sum_q p_q log p_q of softmax(y), a class with p_q = 0 adding exactly 0
    rank[b,s]      = #{q : y_q > y_t} + #{q < t : y_q == y_t}
    seq_nll[b]     = -sum_s logp[b,s]
    seq_correct[b] = #{s : rank[b,s] == 0}

In float64 two different fp32 logits stay different after the division, so the order of y is the order of the logits."""
import torch


def clamp_target(target: torch.Tensor, Q: int) -> torch.Tensor:
    return target.to(torch.int64).clamp(0, Q - 1)


def score(logits: torch.Tensor, target: torch.Tensor, temperature: float = 1.0) -> dict:
    """logits (B, Q, S) of any float type, target (B, S) integers -> dict of float64 / int64 tensors on logits' device."""
    B, Q, S = logits.shape
    y = logits.double() / float(temperature)
    t = clamp_target(target, Q).to(y.device)
    m = y.amax(1, keepdim=True)
    d = y - m                                            # <= 0; -inf for a masked class
    e = torch.exp(d)
    # logsumexp - m as log(k) + log1p(rest / k), k classes at the maximum and `rest` the sum over the others: a column
    # whose other classes add up to less than 1e-16 keeps a log-sum of the right size instead of 0
    top = d == 0
    k = top.sum(1).double()
    lse = torch.log(k) + torch.log1p(torch.where(top, torch.zeros_like(e), e).sum(1) / k)
    yt = y.gather(1, t[:, None, :])[:, 0]
    logp = (yt - m[:, 0]) - lse
    logq = d - lse[:, None, :]                           # log p_q
    plogp = torch.where(e > 0, (e / e.sum(1, keepdim=True)) * logq, torch.zeros_like(e))
    entropy = -plogp.sum(1)
    q = torch.arange(Q, device=y.device)[None, :, None]
    above = (y > yt[:, None, :]) | ((y == yt[:, None, :]) & (q < t[:, None, :]))
    rank = above.sum(1)
    return {"logp": logp, "entropy": entropy, "rank": rank, "seq_nll": -logp.sum(1),
            "seq_correct": (rank == 0).sum(1)}
