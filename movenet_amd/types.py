"""Layout contract of the model API (drop-in for /root/reference/movenet/types.py:4-5).

The reference spells these with ``torchtyping.TensorType[...]``, which it uses in annotations only
(movenet/wavenet.py:15, :162).  torchtyping is not a dependency here: the aliases are
``typing.Annotated[torch.Tensor, <dimension names>]`` -- the same information for a reader or a
type checker, nothing at run time.  Layouts:

* ``AudioTensor``: ``(batch, channels, frames)`` -- one-hot mu-law classes on ``channels``,
  time contiguous;
* ``VideoTensor``: ``(batch, frames, height, width, channels)`` -- 64 x 64 grayscale frames.
"""
from typing import Annotated, NamedTuple

import torch

AudioTensor = Annotated[torch.Tensor, ("batch", "channels", "frames")]
VideoTensor = Annotated[torch.Tensor, ("batch", "frames", "height", "width", "channels")]


class PitchDistance(NamedTuple):
    """What ``WaveNet.pitch_distance`` returns, one value per sequence (``movenet_amd.wavenet`` exports it beside
    ``SpectralDistance``)."""
    f0_rmse_cents: torch.Tensor  # (B,) float64 RMS of 1200 log2(F0_generated / F0_source) over voiced_frames; 0.0 with none
    voiced_frames: torch.Tensor  # (B,) int32 frames voiced in both tracks
    vuv_errors: torch.Tensor     # (B,) int32 frames voiced in exactly one of them
    gross_errors: torch.Tensor   # (B,) int32 voiced_frames whose periods differ by more than gross_ratio
    frames: torch.Tensor         # (B,) int32 frames that were compared


__all__ = ["AudioTensor", "VideoTensor", "PitchDistance"]
