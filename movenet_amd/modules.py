"""The reference's five block classes (drop-in names for movenet/modules.py:15-142), callable and trainable on the GPU.

``movenet_amd.wavenet.WaveNet`` is assembled from these exactly as the reference assembles its model
(movenet/wavenet.py:119-123): same constructor signatures, same attribute names, same registration
order -- so ``state_dict`` keys, parameter shapes and the default initialisation drawn under a given
``torch.manual_seed`` are the reference's.

Each block's ``forward`` has the reference's semantics and runs on HIP kernels of its own (``mvn_block_*``,
csrc/blocks.hip) behind a ``torch.autograd.Function`` of ``movenet_amd.ops``: fp32 ``(batch, channels, frames)``
tensors on the GPU, differentiable with respect to the input, the context and every parameter.  So a block can be
called, composed into another network and back-propagated through::

    stack = ResidualConvStack(10, 3, 64, 64).cuda()
    skips = stack(causal_conv(x), None, skip_size)        # (30, batch, 64, skip_size)
    logits = my_head(skips.sum(0))

``WaveNet.forward`` / ``generate`` / the trainer do NOT go through these methods: they keep calling the fused
whole-model kernels (``mvn_forward``, ``mvn_backward``, ``mvn_generate``), and a model's ``forward_precision`` does not
reach the blocks, whose products are fp32-class throughout.  Two stated deviations from the reference:

* ``GatedResidualConv1d`` raises ``ValueError`` for a negative ``skip_size`` (the reference would silently drop leading
  columns); 0 and values above ``T - d`` return all ``T - d`` columns, as Python slicing does.
* A context longer than the layer's output is used by its LAST ``T - d`` columns (right-aligned, the definition the
  model and the oracle use); the reference's own layer runs only at ``Tc == T - d``.  A shorter one raises ``ValueError``.

There is no CPU path: CPU tensors, or a block whose parameters live on the CPU, raise ``RuntimeError``.
"""
from __future__ import annotations

from typing import List

import torch.nn as nn

__all__ = ["CausalConv1d", "DilatedCausalConv1d", "GatedResidualConv1d", "ResidualConvStack", "DenseConv"]


class _Block(nn.Module):
    def _require_gpu(self, *tensors):
        on_cpu = [t for t in tensors if t is not None and not t.is_cuda] or [p for p in self.parameters() if not p.is_cuda]
        if on_cpu:
            raise RuntimeError(
                f"{type(self).__name__} holds parameters under the reference's names and its arithmetic runs in HIP kernels: "
                "the blocks run on GPU tensors only (move the block and its inputs to the device; there is no CPU path, "
                "see movenet_amd/modules.py)")

    def _require_two_taps(self, kernel_size):
        if kernel_size != 2:
            raise NotImplementedError(f"{type(self).__name__}: kernel_size = {kernel_size}; the kernels implement "
                                      "kernel_size == 2, the only value the model uses")


class CausalConv1d(_Block):
    """movenet/modules.py:15-30: ``Conv1d(in, out, k, padding=1, bias)`` whose last output column is dropped."""

    def __init__(self, input_channels, out_channels, kernel_size=2, bias=False):
        super().__init__()
        self.kernel_size = kernel_size
        self.conv = nn.Conv1d(input_channels, out_channels, kernel_size, padding=1, bias=bias)

    def forward(self, x):
        from . import ops
        self._require_two_taps(self.kernel_size)
        self._require_gpu(x)
        return ops.block_causal_conv(x, self.conv.weight, self.conv.bias)


class DilatedCausalConv1d(_Block):
    """movenet/modules.py:33-46: ``Conv1d(C, C, k, dilation=d, padding=0, bias)``."""

    def __init__(self, channels, dilation=1, kernel_size=2, bias=False):
        super().__init__()
        self.conv = nn.Conv1d(channels, channels, kernel_size, dilation=dilation, padding=0, bias=bias)

    def forward(self, x):
        from . import ops
        self._require_two_taps(self.conv.kernel_size[0])
        self._require_gpu(x)
        return ops.block_dilated_conv(x, self.conv.weight, self.conv.bias, self.conv.dilation[0])


class GatedResidualConv1d(_Block):
    """movenet/modules.py:49-93: filter / gate dilated convs, the two context 1x1 convs, residual and skip 1x1 convs."""

    def __init__(self, residual_channels, skip_channels, dilation):
        super().__init__()
        self.conv_filter = DilatedCausalConv1d(residual_channels, dilation=dilation)
        self.conv_gate = DilatedCausalConv1d(residual_channels, dilation=dilation)
        self.context_conv_filter = nn.Conv1d(residual_channels, residual_channels, 1)
        self.context_conv_gate = nn.Conv1d(residual_channels, residual_channels, 1)
        self.conv_residual = nn.Conv1d(residual_channels, residual_channels, 1)
        self.conv_skip = nn.Conv1d(residual_channels, skip_channels, 1)

    def _block_params(self):
        """The layer's tensors in ``ops.GATED_PARAMS`` order."""
        return [self.conv_filter.conv.weight, self.conv_filter.conv.bias, self.conv_gate.conv.weight,
                self.conv_gate.conv.bias, self.context_conv_filter.weight, self.context_conv_filter.bias,
                self.context_conv_gate.weight, self.context_conv_gate.bias, self.conv_residual.weight,
                self.conv_residual.bias, self.conv_skip.weight, self.conv_skip.bias]

    def forward(self, input, context, skip_size):
        """Returns ``(residual (B, C, T - d), skip (B, K, skip_size))``."""
        from . import ops
        self._require_two_taps(self.conv_filter.conv.kernel_size[0])
        self._require_gpu(input, context)
        return ops.block_gated_layer(input, context, skip_size, self.conv_filter.conv.dilation[0], self._block_params())


class ResidualConvStack(_Block):
    """movenet/modules.py:96-130: ``stack_size`` cycles of dilations 1, 2, ..., 2^(layer_size - 1)."""

    def __init__(self, layer_size, stack_size, residual_channels, skip_channels):
        super().__init__()
        self.layer_size = layer_size
        self.stack_size = stack_size
        self.conv_layers = nn.ModuleList([
            GatedResidualConv1d(residual_channels, skip_channels, dilation) for dilation in self.dilations
        ])

    @property
    def dilations(self) -> List[int]:
        return [2 ** x for _ in range(self.stack_size) for x in range(self.layer_size)]

    def forward(self, input, context, skip_size):
        """Returns the layers' skips stacked as ``(L, B, K, skip_size)``; a context is ``(B, C, T)``, aligned with
        ``input`` (each layer takes its last columns)."""
        from . import ops
        self._require_gpu(input, context)
        return ops.block_residual_stack(input, context, skip_size, self.dilations,
                                        [layer._block_params() for layer in self.conv_layers])


class DenseConv(_Block):
    """movenet/modules.py:133-142: two 1x1 convs behind leaky ReLUs (the mu-law head)."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv1 = nn.Conv1d(in_channels, out_channels, 1)
        self.conv2 = nn.Conv1d(out_channels, out_channels, 1)

    def forward(self, x):
        from . import ops
        self._require_gpu(x)
        return ops.block_dense_conv(x, self.conv1.weight, self.conv1.bias, self.conv2.weight, self.conv2.bias)
