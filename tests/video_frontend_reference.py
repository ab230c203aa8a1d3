"""The oracle of the video front end (a helper, not a test): what the reference's loader does to decoded frames --
torchvision's ``rgb_to_grayscale`` then ``resize`` to 64 x 64 on uint8 tensors -- restated in plain torch on the CPU
(torchvision is absent; it calls exactly these expressions).

* ``gray``: ``(0.2989 * r + 0.587 * g + 0.114 * b).to(torch.uint8)`` on uint8 planes: fp32 products and sums, left to
  right, each rounded; the cast truncates (255, 255, 255 -> 254.9745 -> 254).
* ``resize``: ``torch.nn.functional.interpolate(l.float(), size=(64, 64), mode="bilinear", align_corners=False,
  antialias=A)``, ``torch.round`` (half to even), cast to uint8.
* ``frontend`` returns output A (the chain in fp32: the definition), output B (the same chain with the interpolation
  in float64, before rounding) and ``d = max |fp32 - fp64|`` of the values before rounding.
"""
from __future__ import annotations

import numpy as np
import torch

SIZE = 64


def gray(frames: torch.Tensor) -> torch.Tensor:
    """(..., H, W, 3) uint8 -> (..., H, W) uint8; (..., H, W) uint8 given with ``channels=1`` is not passed here."""
    r, g, b = frames[..., 0], frames[..., 1], frames[..., 2]
    return (0.2989 * r + 0.587 * g + 0.114 * b).to(torch.uint8)


def _interp(l: torch.Tensor, antialias: bool, dtype) -> torch.Tensor:
    """(F, H, W) uint8 -> (F, 64, 64) ``dtype`` before rounding."""
    return torch.nn.functional.interpolate(l.to(dtype)[:, None], size=(SIZE, SIZE), mode="bilinear",
                                           align_corners=False, antialias=bool(antialias))[:, 0]


def frontend(frames, antialias: bool = False, chunk: int = 512):
    """``frames``: (F, H, W, 3) or (F, H, W) uint8 (numpy or torch).  Returns (A, B, d): A (F, 64, 64) uint8 levels of
    the fp32 chain, B (F, 64, 64) float64 values before rounding with the interpolation in float64, d the largest
    |fp32 - fp64| before rounding."""
    frames = torch.as_tensor(np.asarray(frames) if not torch.is_tensor(frames) else frames)
    if frames.dtype != torch.uint8 or frames.dim() not in (3, 4) or (frames.dim() == 4 and frames.shape[-1] != 3):
        raise ValueError(f"uint8 (F, H, W, 3) or (F, H, W) expected, got {frames.dtype} {tuple(frames.shape)}")
    A, B, d = [], [], 0.0
    for s in range(0, frames.shape[0], chunk):
        l = frames[s:s + chunk]
        if l.dim() == 4:
            l = gray(l)
        a32 = _interp(l, antialias, torch.float32)
        b64 = _interp(l, antialias, torch.float64)
        d = max(d, float((a32.double() - b64).abs().max()))
        A.append(torch.round(a32).to(torch.uint8))
        B.append(b64)
    return torch.cat(A), torch.cat(B), d


def levels(frames, antialias: bool = False) -> torch.Tensor:
    """Output A alone."""
    return frontend(frames, antialias)[0]


def round_half_even(b: torch.Tensor) -> torch.Tensor:
    return torch.round(b)


def tie_distance(b: torch.Tensor) -> torch.Tensor:
    """Distance of every value from the nearest rounding tie (k + 0.5)."""
    return ((b - torch.floor(b)) - 0.5).abs()


def subsample_indices(F: int, n: int) -> np.ndarray:
    """pytorchvideo's uniform_temporal_subsample: linspace, clamp, truncate."""
    return np.clip(np.linspace(0, F - 1, n), 0, F - 1).astype(np.int64)
