"""CPU emulation of video-conditioned bf16 training (mvn_forward_bf16_ctx / mvn_backward_bf16_ctx): bf16_emulation's
layer with the context term of every gated layer.  Forward the term is conv1d(bf(ctx), bf(Wc)) -- one more K block of the
f | g contraction, its operands rounded once -- plus the fp32 bias.  Backward it is NOT a product of rounded operands:
the context pass forms dctx = Wc^T dfg, dWc = sum dfg ctx^T and dbc = sum dfg in fp32 from the unrounded df | dg, the
unrounded ctx and the unrounded weights, so the term is a custom autograd function that sits outside ``_RoundGrad``.
``ctx``: the (B, C, T) context, an argument that takes gradients."""
from __future__ import annotations

from typing import Dict

import torch
import torch.nn.functional as F

from bf16_emulation import _conv, _key, bf, grads_of  # noqa: F401  (bf and grads_of: re-exported for the tests)
from oracle import wavenet_oracle as O


class _ContextTerm(torch.autograd.Function):
    @staticmethod
    def forward(fctx, c, w):
        fctx.save_for_backward(c, w)
        return F.conv1d(bf(c), bf(w))

    @staticmethod
    def backward(fctx, g):
        c, w = fctx.saved_tensors
        return torch.einsum("oi,bot->bit", w[:, :, 0], g), torch.einsum("bot,bit->oi", g, c)[:, :, None]


def _context_term(sd, l: int, which: str, c: torch.Tensor) -> torch.Tensor:
    return (_ContextTerm.apply(c, sd[_key(l, f"context_conv_{which}.weight")])
            + sd[_key(l, f"context_conv_{which}.bias")][None, :, None])


def logits(sd: Dict[str, torch.Tensor], dims: O.Dims, audio: torch.Tensor, context: torch.Tensor) -> torch.Tensor:
    h = O.causal_conv(sd, audio)
    assert context.size() == h.size()
    skip_size = dims.output_size(h.size(2))
    skips = []
    for l, d in enumerate(dims.dilations):
        f = _conv(h, sd[_key(l, "conv_filter.conv.weight")], dilation=d)
        g = _conv(h, sd[_key(l, "conv_gate.conv.weight")], dilation=d)
        c = context[:, :, -f.size(2):]  # (right-aligned with f | g, like the residual input: the oracle's gated_layer)
        f = f + _context_term(sd, l, "filter", c)
        g = g + _context_term(sd, l, "gate", c)
        z = torch.tanh(f) * torch.sigmoid(g)
        res = _conv(z, sd[_key(l, "conv_residual.weight")], sd[_key(l, "conv_residual.bias")])
        s = _conv(z, sd[_key(l, "conv_skip.weight")], sd[_key(l, "conv_skip.bias")])
        h = res + h[:, :, -res.size(2):]
        skips.append(s[:, :, -skip_size:])
    return O.dense_head(sd, torch.sum(torch.stack(skips), dim=0))
