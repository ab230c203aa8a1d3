"""CPU emulation of the bf16 training mode (mvn_forward_bf16 / mvn_backward_bf16) built on the fp32 oracle's
arithmetic: every product of a gated layer takes bf16-rounded operands (round to nearest even) -- x(t), x(t - d),
z and the four weights forward; the gradient arriving at each layer conv's output backward, so that dz, the input
gradient and the weight gradients are products of rounded operands too -- with fp32 sums; biases, the gate, the
residual add, the skip sum, the embedding and the head stay fp32.  It is the yardstick the GPU tests calibrate
their tolerances against (accumulation order alone moves values across bf16 rounding boundaries, so no test can
pin the kernels to it element-wise)."""
from __future__ import annotations

from typing import Dict

import torch
import torch.nn.functional as F

from oracle import wavenet_oracle as O


def bf(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(x.dtype)


class _RoundGrad(torch.autograd.Function):
    """Identity forward; rounds the incoming gradient to bf16 (the operand of the products behind it)."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return bf(g)


def _rounded(x: torch.Tensor) -> torch.Tensor:
    return x + (bf(x) - x).detach()  # bf16 value forward, the gradient passes unchanged


def _conv(x, w, b=None, dilation=1):
    y = _RoundGrad.apply(F.conv1d(_rounded(x), _rounded(w), None, dilation=dilation))
    return y if b is None else y + b[None, :, None]


def _key(l: int, name: str) -> str:
    return f"residual_conv_stack.conv_layers.{l}.{name}"


def logits(sd: Dict[str, torch.Tensor], dims: O.Dims, audio: torch.Tensor) -> torch.Tensor:
    h = O.causal_conv(sd, audio)
    skip_size = dims.output_size(h.size(2))
    skips = []
    for l, d in enumerate(dims.dilations):
        f = _conv(h, sd[_key(l, "conv_filter.conv.weight")], dilation=d)
        g = _conv(h, sd[_key(l, "conv_gate.conv.weight")], dilation=d)
        z = torch.tanh(f) * torch.sigmoid(g)
        res = _conv(z, sd[_key(l, "conv_residual.weight")], sd[_key(l, "conv_residual.bias")])
        s = _conv(z, sd[_key(l, "conv_skip.weight")], sd[_key(l, "conv_skip.bias")])
        h = res + h[:, :, -res.size(2):]
        skips.append(s[:, :, -skip_size:])
    return O.dense_head(sd, torch.sum(torch.stack(skips), dim=0))


def grads_of(fn, sd: Dict[str, torch.Tensor]):
    """(value, {name: grad}) of the scalar fn(params) over a fresh copy of the parameters."""
    params = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    val = fn(params)
    val.backward()
    return val.detach(), {k: p.grad for k, p in params.items() if p.grad is not None}
