"""CPU emulation of the labelled bf16 training mode (mvn_forward_bf16_global / mvn_backward_bf16_global): bf16_emulation's
``logits`` with the class label's term of every gated layer, f += (Wcf_l e + bcf_l)[:, :, None] and the same for g.  The
term is fp32 and un-rounded, forward and backward: nothing of it enters a product of the layer kernels, and its
gradients are the fp32 row sums of df | dg.  ``e``: the (B, C) global vectors, an argument that takes gradients."""
from __future__ import annotations

from typing import Dict

import torch

from bf16_emulation import _conv, _key, bf, grads_of  # noqa: F401  (bf and grads_of: re-exported for the tests)
from oracle import wavenet_oracle as O


def _label_term(sd, l: int, which: str, e: torch.Tensor) -> torch.Tensor:
    w = sd[_key(l, f"context_conv_{which}.weight")][:, :, 0]
    return (e @ w.t() + sd[_key(l, f"context_conv_{which}.bias")])[:, :, None]


def logits(sd: Dict[str, torch.Tensor], dims: O.Dims, audio: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    h = O.causal_conv(sd, audio)
    skip_size = dims.output_size(h.size(2))
    skips = []
    for l, d in enumerate(dims.dilations):
        f = _conv(h, sd[_key(l, "conv_filter.conv.weight")], dilation=d) + _label_term(sd, l, "filter", e)
        g = _conv(h, sd[_key(l, "conv_gate.conv.weight")], dilation=d) + _label_term(sd, l, "gate", e)
        z = torch.tanh(f) * torch.sigmoid(g)
        res = _conv(z, sd[_key(l, "conv_residual.weight")], sd[_key(l, "conv_residual.bias")])
        s = _conv(z, sd[_key(l, "conv_skip.weight")], sd[_key(l, "conv_skip.bias")])
        h = res + h[:, :, -res.size(2):]
        skips.append(s[:, :, -skip_size:])
    return O.dense_head(sd, torch.sum(torch.stack(skips), dim=0))
