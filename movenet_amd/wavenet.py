"""MI355X-native WaveNet decoder behind the reference's model API.

Drop-in for ``movenet.wavenet.WaveNet`` (/root/reference/movenet/wavenet.py:50-239):
same constructor, same public attributes and module constants, same
``forward`` / ``generate`` / ``receptive_fields`` / ``compute_output_size`` /
``upsample_video`` signatures, same ``state_dict`` keys (so reference
checkpoints load with ``load_state_dict``), same exception types.  The
arithmetic runs in hand-written HIP kernels through the C ABI of
``include/movenet_hip.h``; tensors must live on an MI355X -- there is no CPU
or PyTorch-op fallback.

The sub-modules (``movenet_amd.modules``: the reference's five block classes by name)
hold the parameters under the reference's names and draw the same default
initialisation in the same order, so that the same ``torch.manual_seed`` yields the
same initial weights as the reference; their own ``forward`` is never used.
"""
from __future__ import annotations

import math
import sys
from typing import List, NamedTuple, Optional

import numpy as np
import torch
import torch.nn as nn

from . import _native as N
from .modules import CausalConv1d, DenseConv, ResidualConvStack
from .types import AudioTensor, PitchDistance, VideoTensor  # noqa: F401  (re-exported like movenet/wavenet.py:15)
from .generation import (GroupedGenerator, HostWords, PipeHandoffTimeout, RingGenerator, _require_gpu,
                         _stream_ptr, auto_plan, max_pipe_batch)

# module constants other movenet files import (movenet/wavenet.py:27-31)
MAX_AUDIO_FRAMES = 160000
MAX_VIDEO_FRAMES = 160
VIDEO_KERNEL_SIZE = (1, 64, 64)
UPSAMPLE_STRIDE = 10
MAX_LOCAL_WINDOW = 16  # frames of context on each side of local_conv (33 taps: mvn_upsample_features_win's limit)


def upsample_kernel_size_solver(in_size, out_size, stride=1, padding=0, output_padding=0, dilation=1):
    """Kernel size k with (in-1)*stride - 2*padding + dilation*(k-1) + output_padding + 1 == out
    (the ConvTranspose1d length formula); same contract as movenet/wavenet.py:34-47."""
    span = out_size - 1 - output_padding - (in_size - 1) * stride + 2 * padding
    return (int(span / dilation + 1),)


class _ScoreFields(NamedTuple):
    logp: torch.Tensor             # (B, S) log p(x_t | x_<t, conditioning), nats
    nll: torch.Tensor              # (B,)   -logp.sum(1)
    bits_per_sample: torch.Tensor  # (B,)   nll / (positions ln 2)
    accuracy: torch.Tensor         # (B,)   share of positions whose sample is the first maximum
    entropy: Optional[torch.Tensor] = None  # (B, S) entropy of each predictive distribution, nats (on request)
    rank: Optional[torch.Tensor] = None     # (B, S) int32 rank of the sample in it, 0 = likeliest (on request)


class ScoreResult(_ScoreFields):
    """What ``WaveNet.score`` returns (S = T - RF scored positions per sequence): the six fields above, as a tuple,
    and ``positions``, (B,) int32 -- how many positions of each sequence were scored (S, or fewer with ``lengths``).
    ``positions`` is an attribute beside the tuple: code that unpacks the six fields keeps working."""
    positions: Optional[torch.Tensor] = None

    def __new__(cls, *args, positions=None, **kwargs):
        self = super().__new__(cls, *args, **kwargs)
        self.positions = positions
        return self


class SpectralDistance(NamedTuple):
    """What ``WaveNet.spectral_distance`` returns, one value per sequence."""
    lsd_db: torch.Tensor   # (B,) float64 log-spectral distance of the log-mel frames, dB
    l1: torch.Tensor       # (B,) float64 mean absolute difference of the log-mel frames, nats
    frames: torch.Tensor   # (B,) int32 frames that were compared
    per_frame: Optional[torch.Tensor] = None  # (B, F) float32 distance of each frame, dB; 0 outside the span (on request)


class WaveNet(nn.Module):
    def __init__(self, layer_size: int, stack_size: int, input_channels: int,
                 residual_channels: int = 16, skip_channels: int = 16,
                 context_in_channels: int = 1, global_classes: int = 0, local_channels: int = 0,
                 local_hop: int = 0, local_window: int = 0):
        """``global_classes`` (an extension behind the reference's arguments; 0, the default, is the reference's
        module to the bit): G > 0 registers ``global_embedding.weight`` (G, residual_channels) behind every other
        parameter and makes ``global_features`` a required input of ``forward`` / ``generate``.

        ``local_channels`` / ``local_hop`` (likewise an extension; 0: off, the module unchanged): M > 0 registers
        ``local_conv = nn.Conv1d(M, residual_channels, 1)`` behind every other parameter, ``global_embedding``
        included, and makes ``local_features`` -- (B, M, F) feature frames ``local_hop`` samples apart, e.g.
        ``ops.logmel`` -- a required input of ``forward`` / ``score`` / ``classify``, and ``generate_local_features`` one
        of ``generate``.

        ``local_window`` (0, the default: the module above, same shapes, keys and RNG draws): k > 0 makes it
        ``local_conv = nn.Conv1d(M, residual_channels, 2 k + 1)`` -- a frame's projection sees k frames on each side, the
        edge frames repeated past the ends of ``local_features``.  At most ``MAX_LOCAL_WINDOW`` = 16."""
        super().__init__()
        if isinstance(global_classes, bool) or not isinstance(global_classes, int) or global_classes < 0:
            raise ValueError(f"global_classes must be an integer >= 0, got {global_classes!r}")
        for name, v in (("local_channels", local_channels), ("local_hop", local_hop)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 0:
                raise ValueError(f"{name} must be an integer >= 0, got {v!r}")
        if (local_channels > 0) != (local_hop > 0):
            raise ValueError("local_channels and local_hop go together: both above 0, or both 0 (off), got "
                             f"{local_channels} and {local_hop}")
        self.local_channels, self.local_hop = local_channels, local_hop
        self.local_window = self._checked_local_window(local_window, local_channels)
        self.global_classes = global_classes
        self.layer_size = layer_size
        self.stack_size = stack_size
        self.input_channels = input_channels
        self.residual_channels = residual_channels
        self.skip_channels = skip_channels
        C, K, Q = residual_channels, skip_channels, input_channels

        # registration order == the reference's (wavenet.py:94-123): same RNG draws
        self.video_conv = nn.Conv3d(context_in_channels, C, VIDEO_KERNEL_SIZE)
        n_up = math.ceil(np.log10(MAX_AUDIO_FRAMES / MAX_VIDEO_FRAMES) + 1)
        sizes = np.geomspace(MAX_VIDEO_FRAMES, MAX_AUDIO_FRAMES, num=n_up).astype(int)
        self.video_transpose = nn.Sequential(*[
            nn.ConvTranspose1d(C, C, upsample_kernel_size_solver(a, b, stride=UPSAMPLE_STRIDE),
                               stride=UPSAMPLE_STRIDE)
            for a, b in zip(sizes[:-1], sizes[1:])
        ])
        self.causal_conv = CausalConv1d(Q, C)
        self.residual_conv_stack = ResidualConvStack(layer_size, stack_size, C, K)
        self.dense_conv = DenseConv(K, Q)
        if global_classes > 0:  # (registered last: the draws of every other parameter under a seed do not move)
            self.global_embedding = nn.Embedding(global_classes, C)
        if local_channels > 0:  # (behind everything else, for the same reason)
            self.local_conv = nn.Conv1d(local_channels, C, 2 * self.local_window + 1)
        # "auto" (default): global conditioning takes the fast path where it exists (C = K = 64, fp32, no video: one
        # bias vector per layer and sequence); "context": always the general path, the label as a constant context
        self._global_path = "auto"

        self._dims = N.make_dims(layer_size, stack_size, Q, C, K)
        self._gen_variant = N.GEN_AUTO
        self.last_generate_fallback = None  # variant a timed-out PIPE call was rerun on
        # "fp32" (default) or "fp16": fp16 operands / fp32 accumulation in every product of
        # forward() (mvn_forward_f16, any dims; inference only -- training stays fp32), or "bf16":
        # bf16 operands / fp32 accumulation in the layers' products, forward AND backward
        # (mvn_forward_bf16 / mvn_backward_bf16: audio-only, residual = skip channels = 64)
        self.forward_precision = "fp32"
        # under forward_precision "bf16": also run a video context on bf16 operands (mvn_forward_bf16_ctx /
        # mvn_backward_bf16_ctx); False (default): a context is refused, as before.  Labels with video ride in the context
        self.bf16_context = False
        self._gen_sampling = "reference"
        self._gen_top_k, self._gen_top_p = 0, 1.0
        self._loss_rule = "reference"

    @staticmethod
    def _checked_local_window(local_window, local_channels) -> int:
        if isinstance(local_window, bool) or not isinstance(local_window, int) or local_window < 0:
            raise ValueError(f"local_window must be an integer >= 0, got {local_window!r}")
        if local_window > MAX_LOCAL_WINDOW:
            raise ValueError(f"local_window must be at most {MAX_LOCAL_WINDOW}, got {local_window}")
        if local_window > 0 and local_channels <= 0:
            raise ValueError(f"local_window = {local_window} needs local_channels: there is no local_conv to widen")
        return local_window

    def set_local_conditioning(self, local_channels: int, local_hop: int, local_window: int = 0) -> None:
        """Give the model the ``local_conv`` of ``WaveNet(local_channels=..., local_hop=..., local_window=...)`` (what
        ``checkpoint.load_into`` does for a checkpoint that records one): a new ``nn.Conv1d`` behind every other
        parameter, on their device, unless the model already has one of that width and window; ``local_hop`` is set
        either way."""
        if local_channels < 1 or local_hop < 1:
            raise ValueError(f"local_channels and local_hop must be above 0, got {local_channels} and {local_hop}")
        local_window = self._checked_local_window(local_window, local_channels)
        if int(getattr(self, "local_channels", 0)) != local_channels or \
                int(getattr(self, "local_window", 0)) != local_window:
            if hasattr(self, "local_conv"):
                del self.local_conv
            ref = self.causal_conv.conv.weight
            self.local_conv = nn.Conv1d(local_channels, self.residual_channels,
                                        2 * local_window + 1).to(device=ref.device, dtype=ref.dtype)
        self.local_channels, self.local_hop, self.local_window = int(local_channels), int(local_hop), local_window

    # ---- precision of generate() ----------------------------------------
    @property
    def generate_precision(self) -> str:
        """"fp32" (default: the reference's own precision) or "fp16": fp16 operands with fp32
        accumulation in every product of the autoregressive path (BASELINE configs[4]; the
        reference's precedent for reduced precision is torch.autocast, movenet/trainer.py:124).
        fp16 exists for C = K = 128, Q = 256 (kernel MVN_GEN_PIPE_F16)."""
        return "fp16" if self._gen_variant == N.GEN_PIPE_F16 else "fp32"

    @generate_precision.setter
    def generate_precision(self, value: str) -> None:
        if value == "fp32":
            self._gen_variant = N.GEN_AUTO
        elif value == "fp16":
            N.check(N.lib().mvn_gen_variant(self._dims, N.GEN_PIPE_F16, 1), "generate_precision = 'fp16'")
            self._gen_variant = N.GEN_PIPE_F16
        else:
            raise ValueError(f"generate_precision must be 'fp32' or 'fp16', got {value!r}")

    # ---- what a sampled generate() step draws from -----------------------
    @property
    def generate_sampling(self) -> str:
        """"reference" (default: the reference's rule, softmax(softmax(logits) / T) -- its second softmax
        sees inputs in [0, 1], so the draw is close to uniform whatever the model has learned) or "model":
        the distribution the network was trained to predict, softmax(logits / T).  Only steps with
        temperature > 0 consult it; greedy decoding is the same under both."""
        return getattr(self, "_gen_sampling", "reference")  # (a module pickled before the attribute existed)

    @generate_sampling.setter
    def generate_sampling(self, value: str) -> None:
        N.sampling_rule(value)  # ValueError for anything else
        self._gen_sampling = value

    # ---- truncation of a sampled generate() step --------------------------
    @property
    def generate_top_k(self) -> int:
        """0 (default: off) or k: a sampled step draws among the k likeliest classes only (ties at the k-th weight
        all kept; k >= input_channels is the same as off).  Greedy decoding ignores it."""
        return getattr(self, "_gen_top_k", 0)  # (a module pickled before the attribute existed)

    @generate_top_k.setter
    def generate_top_k(self, value: int) -> None:
        self._gen_top_k = N.truncation(value, 1.0)[0]  # ValueError for anything else

    @property
    def generate_top_p(self) -> float:
        """1.0 (default: off) or p in (0, 1): a sampled step draws from the smallest head of the distribution that
        holds p of its mass (nucleus sampling), applied after ``generate_top_k``.  Greedy decoding ignores it."""
        return getattr(self, "_gen_top_p", 1.0)

    @generate_top_p.setter
    def generate_top_p(self, value: float) -> None:
        self._gen_top_p = N.truncation(0, value)[1]

    # ---- the Philox key(s) of generate() -----------------------------------
    @property
    def generate_seed(self):
        """None (default: every ``generate()`` call draws a key from torch's generator), an int, or a sequence of B
        ints, one key per sequence of the batch (``generate()`` refuses another length)."""
        return getattr(self, "_gen_seed", None)  # (a module pickled before the attribute existed)

    @generate_seed.setter
    def generate_seed(self, value) -> None:
        if value is not None:
            N.seq_sampling_array(len(value) if N.any_per_sequence(value) else 1, self.input_channels, 1.0, 0, 1.0, value)
        self._gen_seed = value

    # ---- classifier-free guidance of generate() ----------------
    @property
    def generate_guidance(self):
        """1.0 (default: off -- ``generate()`` takes the unguided path untouched), a float s, or a sequence of B floats,
        one scale per sequence of the batch (``generate()`` refuses another length).  The network then runs twice per
        step, with the label's vector and with the zero vector in its place (the "no label" condition label dropout
        trains: ``global_dropout``), and the step draws from l_c + (s - 1) (l_c - l_u).  Needs a model built with
        ``global_classes``; a value that is not finite is a ValueError."""
        return getattr(self, "_gen_guidance", 1.0)

    @generate_guidance.setter
    def generate_guidance(self, value) -> None:
        scales = N.guidance_scales(len(value) if N.any_per_sequence(value) else 1, value)  # ValueError for anything else
        if int(getattr(self, "global_classes", 0)) <= 0 and any(s != 1.0 for s in scales):
            raise ValueError("generate_guidance needs a model built with global_classes (there is no label to guide by)")
        self._gen_guidance = list(scales) if N.any_per_sequence(value) else scales[0]

    # ---- the pre-emphasis the model's classes were made under -------------
    @property
    def preemphasis(self) -> float:
        """0.0 (default: off) or the coefficient a in (0, 1) of the pre-emphasis the training audio went through
        (``WavFolderLoader(preemphasis=a)``): ``generate_stream`` then hands its PCM out through the inverse filter
        (``ops.pcm16_chunk(deemphasis=a)``).  Not part of ``state_dict``: a checkpoint carries it as a record of its
        own, which ``checkpoint.load_into`` sets here.  ``generate()`` returns classes and does not consult it."""
        return getattr(self, "_preemphasis", 0.0)  # (a module pickled before the attribute existed)

    @preemphasis.setter
    def preemphasis(self, value: float) -> None:
        N.emphasis(value)  # ValueError for anything outside [0, 1)
        self._preemphasis = float(value)  # (as given: the kernels take its float32 value)

    # ---- the feature frames generate() runs under -------------------
    @property
    def generate_local_features(self):
        """None (default) or the (B, local_channels, F) feature frames ``generate()`` conditions on -- what ``forward``
        takes as ``local_features``, with frames for every sample asked for.  Required (ValueError at ``generate()``) on
        a model built with ``local_channels``; setting it on a model without is a ValueError.  ONE call uses it: the
        next ``generate()`` takes the frames and leaves the setting at None again (also when it raises), so frames
        of one prompt are never reused silently for another, no device tensor stays alive behind the module and none
        is pickled with it between calls.  Set it before every ``generate()``."""
        return getattr(self, "_gen_local_features", None)

    @generate_local_features.setter
    def generate_local_features(self, value) -> None:
        if value is not None:
            if int(getattr(self, "local_channels", 0)) <= 0:
                raise ValueError("generate_local_features set on a model built without local_channels")
            if not torch.is_tensor(value) or value.dim() != 3 or value.shape[1] != self.local_channels \
                    or not value.is_floating_point():
                raise ValueError(f"generate_local_features must be a (batch, {self.local_channels}, frames) float tensor")
        self._gen_local_features = value

    # ---- label dropout of train-mode forward() ---------------------------------
    @property
    def global_dropout(self) -> float:
        """0.0 (default: off, nothing is drawn) or P in [0, 1]: in TRAIN mode ``forward`` replaces the label's vector
        of each sequence by zeros with probability P -- the mask (``global_dropout_mask``) is drawn from
        ``global_dropout_generator``, a host ``torch.Generator`` (default: one seeded with 0), never from torch's
        global generator.  Eval mode and ``generate()`` never drop."""
        return getattr(self, "_global_dropout", 0.0)

    @global_dropout.setter
    def global_dropout(self, value: float) -> None:
        if isinstance(value, bool) or not isinstance(value, (int, float)) or not 0.0 <= value <= 1.0:
            raise ValueError(f"global_dropout must lie in [0, 1], got {value!r}")
        self._global_dropout = float(value)

    def global_dropout_mask(self, batch: int):
        """The (batch,) float32 host mask of one train step -- 0 where the label is dropped, 1 elsewhere -- or None
        when ``global_dropout`` is 0 (nothing is drawn then)."""
        p = self.global_dropout
        if p <= 0.0:
            return None
        gen = getattr(self, "global_dropout_generator", None)
        if gen is None:
            gen = self.global_dropout_generator = torch.Generator().manual_seed(0)
        return (torch.rand(int(batch), generator=gen) >= p).to(torch.float32)

    # ---- which kernels global conditioning runs ----------------------------
    @property
    def global_path(self) -> str:
        """"auto" (default): the one-vector-per-layer fast path where fp32 runs it, else the general path.  "context":
        force the general path of global conditioning -- the global vector added to the context, the conditioned
        kernels as they are (tests, A/B measurements).  "bias": REQUIRE the one-vector-per-layer path, in whichever
        precision the model runs -- under ``forward_precision = "bf16"`` the labelled bf16 layer kernels
        (mvn_forward_bf16_global / mvn_backward_bf16_global), under fp32 the fast path "auto" prefers; ValueError, before
        anything is launched, where that path does not exist (a video context, residual or skip channels other than
        64, fp16, kernel switches or a shape that mvn_global_fast_path / mvn_global_bf16_path refuses)."""
        return getattr(self, "_global_path", "auto")

    @global_path.setter
    def global_path(self, value: str) -> None:
        if value not in ("auto", "context", "bias"):
            raise ValueError(f"global_path must be 'auto', 'context' or 'bias', got {value!r}")
        self._global_path = value

    # ---- what forward(..., return_loss=True) minimises --------------------
    @property
    def loss_rule(self) -> str:
        """"reference" (default: the reference's loss, cross_entropy applied to the model's PROBABILITIES -- a
        second softmax over values in [0, 1], confined to [ln Q - 1, ln Q] whatever the model predicts) or "model":
        cross_entropy of the head's logits, the mean negative log-likelihood (nats) of softmax(logits) -- the
        distribution ``generate_sampling = "model"`` draws from.  Only ``forward(..., return_loss=True)`` consults
        it; the probabilities and the accuracy it returns are the same under both."""
        return getattr(self, "_loss_rule", "reference")  # (a module pickled before the attribute existed)

    @loss_rule.setter
    def loss_rule(self, value: str) -> None:
        N.loss_rule(value)  # ValueError for anything else
        self._loss_rule = value

    # ---- shape arithmetic (host only) ---------------------------------
    @property
    def receptive_fields(self) -> int:
        # sum of dilations + one more time point per stack (wavenet.py:125-134)
        return sum(self.residual_conv_stack.dilations) + self.stack_size

    def compute_output_size(self, x) -> int:
        out = int(x.size(2)) - self.receptive_fields + 1
        if out < 1:
            raise ValueError(
                "input time steps must be larger than the number of receptive "
                f"fields. Number of input timesteps = {x.size(2)}, "
                f"receptive fields = {self.receptive_fields}"
            )
        return out

    # ---- helpers --------------------------------------------------------
    def _indices_async(self, audio: torch.Tensor):
        """(B,Q,T) one-hot -> ((B,T) int32 indices on device, check token).  Nothing synchronises
        here: the indices' minimum is -1 where a column is not exactly one-hot, and the caller
        reads it (``_all_one_hot``) only AFTER it has enqueued the work that assumes one-hot
        input, so the host never waits on an idle GPU."""
        _require_gpu(audio, "audio")
        if audio.dim() != 3 or audio.size(1) != self.input_channels:
            raise ValueError(f"audio must be (batch, {self.input_channels}, frames), "
                             f"got {tuple(audio.shape)}")
        x = audio.detach().to(torch.float32).contiguous()
        B, Q, T = x.shape
        idx = torch.empty(B, T, dtype=torch.int32, device=x.device)
        with torch.cuda.device(x.device):
            N.check(N.lib().mvn_onehot_to_index(x.data_ptr(), idx.data_ptr(), B, Q, T,
                                                _stream_ptr(x.device)), "mvn_onehot_to_index")
        low = idx.min() if B * T else torch.zeros((), dtype=torch.int32, device=x.device)
        # the minimum goes to pinned host memory from a one-wave kernel queued right behind the
        # kernels that produce it -- ahead of whatever the caller enqueues next (generation.HostWords;
        # nothing of it lives in the module: copy.deepcopy(model) / torch.save(model) keep working)
        return idx, HostWords.publish(low.reshape(1))

    def _all_one_hot(self, check) -> bool:
        """The result of ``_indices_async``'s check: polls the pinned word its publish kernel
        writes (no HIP call, no stream synchronisation: the host waits ONLY for the kernels that
        produced the minimum, not for whatever the caller has enqueued since)."""
        return HostWords.read(check)[0] >= 0

    def _indices_of(self, audio: torch.Tensor, strict: bool = True):
        """(B,Q,T) one-hot -> (B,T) int32 on device (mvn_onehot_to_index).  A column that
        is not one-hot: ValueError when ``strict`` (generation works on class indices),
        else None (forward then takes the dense causal-conv path)."""
        idx, check = self._indices_async(audio)
        if not self._all_one_hot(check):
            if not strict:
                return None
            raise ValueError(
                "movenet_amd.WaveNet expects one-hot audio (movenet/dataset.py:278-289); "
                "a column of the input is not one-hot")
        return idx

    def _one_hot_of(self, idx: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
        B, T = idx.shape
        out = torch.empty(B, self.input_channels, T, dtype=torch.float32, device=idx.device)
        with torch.cuda.device(idx.device):
            N.check(N.lib().mvn_index_to_onehot(idx.data_ptr(), idx.stride(0), out.data_ptr(), B,
                                                self.input_channels, T, _stream_ptr(idx.device)),
                    "mvn_index_to_onehot")
        return out if dtype == torch.float32 else out.to(dtype)

    def _decoder_state(self):
        return {k: v for k, v in self.state_dict().items()
                if not k.startswith(("video_", "global_embedding.", "local_conv."))}

    # ---- model API ------------------------------------------------------
    def upsample_video(self, video):
        """(B, F, 64, 64, Cin) -> (B, C, 1000 F): wavenet.py:149-156 (pinned by fixture G7)."""
        from .ops import upsample_video
        out = upsample_video(self, video)
        assert out.shape[-1] == MAX_AUDIO_FRAMES  # same assert as the reference (:155)
        return out

    def forward(self, audio, video=None, global_features=None, output_unnormalized: bool = True,
                remove_last: bool = True, return_loss: bool = False, target=None, lengths=None, *,
                local_features=None):
        """BUILD DEFINITION for video != None: the reference raises a shape error at
        modules.py:75-77; here the upsampled video is added to the filter
        and gate pre-activations at the same absolute time (right-aligned, like the
        residual input at modules.py:84).

        BUILD DEFINITION for ``global_features`` (the reference declares the argument and never uses it):
        a model built with ``global_classes = G > 0`` owns ``global_embedding.weight`` E of shape (G, C), and sequence
        b carries the vector e_b = E[class_b] for a (B,) integer tensor of classes in [0, G), or row_b @ E for a
        (B, G) float tensor (one-hot, or a mixture).  It enters every gated layer exactly where the context does, as a
        column constant in time: f_l += Wcf_l (ctx + e_b) + bcf_l, g_l += Wcg_l (ctx + e_b) + bcg_l, with ctx the
        up-sampled video or zero.  With G > 0 the argument is required (ValueError); with G = 0 it is ignored.

        ``return_loss=True`` (an extension; the default is the reference's signature and
        result): returns ``(loss, accuracy, probabilities)`` of the trainer's step -- the
        reference's ``output = self(audio, video)``, ``target = audio[:, :, RF:].argmax(1)``,
        ``F.cross_entropy(output, target)`` and accuracy (pytorch_lightning_trainer.py:62-66)
        -- as ONE autograd node (ops.wavenet_forward_loss); going through ``forward`` keeps
        module hooks firing on the fused path.  ``loss_rule = "model"`` makes that loss
        ``F.cross_entropy`` of the logits instead (the property's docstring).

        ``lengths`` (with ``return_loss=True`` only; (B,) host sequence or integer tensor, default None): sequence b
        holds ``lengths[b]`` real samples and padding behind them; loss and accuracy then run over the columns that
        predict a real sample (``ops.valid_columns``), divided by their number, and the padding's columns receive a
        gradient of exactly 0.  Refused together with ``video``: video batches are fixed at
        MAX_AUDIO_FRAMES frames.

        ``local_features`` (a model built with ``local_channels = M > 0``, which requires it; ValueError on a model
        without): (B, M, F) feature frames ``local_hop`` samples apart, F >= (T - 1) // local_hop + 1.  ``local_conv``
        and a linear interpolation between frames make them the (B, C, T) context (``ops.upsample_features``) -- an
        ordinary context: a label joins it as it joins a video's, bf16 needs ``bf16_context``, ``global_path = "bias"``
        refuses it.  Not together with ``video`` (ValueError); ``lengths`` is accepted with it."""
        from .ops import global_vector, plan_sequence, wavenet_forward, wavenet_forward_loss  # HIP full-sequence kernels
        self._lengths_checks(lengths, video, return_loss)
        self._local_checks(audio, video, local_features)
        gvec = global_vector(self, global_features, int(audio.shape[0]))  # (ValueError before anything is launched)
        if gvec is not None and self.training:  # label dropout: both paths below see an ordinary e
            keep = self.global_dropout_mask(int(audio.shape[0]))
            if keep is not None:
                gvec = gvec * keep.to(device=gvec.device, dtype=gvec.dtype)[:, None]
        # (refused before the video encoder / the feature up-sampler runs)
        plan_sequence(self, video is not None or local_features is not None, gvec is not None)
        context = self._context_of(audio, video, local_features)
        if return_loss:
            return wavenet_forward_loss(self, audio, context, target, gvec=gvec, lengths=lengths)
        return wavenet_forward(self, audio, context, output_unnormalized=output_unnormalized,
                               remove_last=remove_last, gvec=gvec)

    @staticmethod
    def _lengths_checks(lengths, video, takes_lengths: bool = True):
        if lengths is None:
            return
        if not takes_lengths:
            raise ValueError("lengths goes with return_loss=True: without the loss there is nothing to leave out")
        if video is not None:
            raise ValueError(f"lengths cannot be combined with video: video batches are fixed at {MAX_AUDIO_FRAMES} "
                             "frames")

    def _local_checks(self, audio, video, local_features, n_total=None):
        """The ValueErrors of ``local_features`` (ops.check_local_features, for the audio's length or ``n_total``),
        before anything is launched; never together with ``video``."""
        from .ops import check_local_features
        if local_features is not None and video is not None:
            raise ValueError("local_features cannot be combined with video: one local context at a time")
        check_local_features(self, local_features, int(audio.shape[0]),
                             int(audio.shape[2]) if n_total is None else int(n_total))

    def _context_of(self, audio, video, local_features, n_total=None):
        """The (B, C, T) local context of a pass: the up-sampled video, the up-sampled feature frames, or None."""
        if local_features is not None:
            from .ops import upsample_features
            return upsample_features(self, local_features, int(audio.shape[2]) if n_total is None else int(n_total))
        return None if video is None else self.upsample_video(video)

    # ---- likelihood of GIVEN audio ---------------------------
    def _score_checks(self, audio, video, global_features, local_features=None):
        """The forward's own refusals, before anything is launched; returns (gvec, the pass's planned mode)."""
        from .ops import global_vector, plan_sequence
        self._local_checks(audio, video, local_features)
        gvec = global_vector(self, global_features, int(audio.shape[0]))
        mode = plan_sequence(self, video is not None or local_features is not None, gvec is not None)
        self.compute_output_size(audio)
        return gvec, mode

    @staticmethod
    def _score_result(raw: dict, positions: int, valid=None) -> "ScoreResult":
        nll = raw["seq_nll"]
        if valid is None:
            return ScoreResult(logp=raw["logp"], nll=nll, bits_per_sample=nll / (max(positions, 1) * math.log(2.0)),
                               accuracy=raw["seq_correct"].to(torch.float32) / max(positions, 1),
                               entropy=raw.get("entropy"), rank=raw.get("rank"),
                               positions=torch.full_like(raw["seq_correct"], positions))
        per = valid.clamp(min=1).to(torch.float32)
        return ScoreResult(logp=raw["logp"], nll=nll, bits_per_sample=nll / (per * math.log(2.0)),
                           accuracy=raw["seq_correct"].to(torch.float32) / per, entropy=raw.get("entropy"),
                           rank=raw.get("rank"), positions=valid)

    def _valid_on_device(self, lengths, audio):
        """``lengths`` -> (B,) int32 valid column counts on the audio's device (None stays None)."""
        from .ops import _valid_for_batch, counts_to_device
        valid = _valid_for_batch(lengths, int(audio.shape[0]), int(audio.shape[2]), self.receptive_fields)
        if valid is None:
            return None
        _require_gpu(audio, "audio")
        return counts_to_device(valid, audio.device)

    @torch.no_grad()
    def score(self, audio, video=None, global_features=None, temperature: float = 1.0, entropy: bool = False,
              rank: bool = False, lengths=None, *, local_features=None) -> "ScoreResult":
        """How likely ``audio`` is under the model: log p(x_t | x_<t, conditioning) of every sample past the
        receptive field, per position and per sequence, from the logits of one forward pass (same checks, same
        kernels, ``forward_precision`` and ``global_path`` as ``forward``; nothing saved, no probability tensor).

        Returns a ``ScoreResult``: ``logp`` (B, T - RF) in nats under softmax(logits / ``temperature``), ``nll`` (B,)
        its negative sum, ``bits_per_sample`` (B,) = nll / ((T - RF) ln 2), ``accuracy`` (B,) the share of positions
        whose sample is the first maximum, and on request ``entropy`` (B, T - RF) of each predictive distribution
        and ``rank`` (B, T - RF) int32 of the sample in it (else None).  ``nll.mean() / (T - RF)`` is the loss
        ``loss_rule = "model"`` reports for the same input.  Label dropout is never applied, the module's training
        flag is left as it is, and ``audio`` must be one-hot (ValueError): its class indices are the targets.

        ``lengths`` (as in ``forward``; default None): sequence b is scored over the positions that predict one of
        its ``lengths[b]`` real samples -- ``positions`` (B,) int32 holds their number, ``bits_per_sample`` and
        ``accuracy`` divide by ``max(positions, 1)``, and the other positions come back as logp = entropy = 0 and
        rank = -1.  Refused together with ``video``.  ``local_features``: as in ``forward``."""
        from .ops import score_temperature, wavenet_score
        temperature = score_temperature(temperature)  # (ValueError before the video encoder runs)
        self._lengths_checks(lengths, video)
        gvec, _ = self._score_checks(audio, video, global_features, local_features)
        valid = self._valid_on_device(lengths, audio)
        context = self._context_of(audio, video, local_features)
        raw = wavenet_score(self, audio, context, gvec, temperature, entropy=entropy, rank=rank, valid=valid)
        return self._score_result(raw, int(audio.shape[2]) - self.receptive_fields, valid)

    def _class_indices(self, x: torch.Tensor, what: str) -> torch.Tensor:
        """(B, T) integer classes, or (B, Q, T) one-hot through ``_indices_of``, as (B, T) int32 on the device."""
        _require_gpu(x, what)
        if x.dim() == 3:
            return self._indices_of(x)
        if x.dim() != 2 or x.is_floating_point() or x.dtype == torch.bool:
            raise ValueError(f"{what} must be (batch, samples) integer classes or (batch, {self.input_channels}, "
                             f"samples) one-hot, got {tuple(x.shape)} {x.dtype}")
        return x.detach().to(torch.int32).contiguous()

    @torch.no_grad()
    def spectral_distance(self, generated, source, lengths=None, skip: Optional[int] = None, per_frame: bool = False, *,
                          n_fft: Optional[int] = None, hop: Optional[int] = None, n_mels: Optional[int] = None,
                          rate: Optional[float] = None, f_min: Optional[float] = None,
                          f_max: Optional[float] = None) -> "SpectralDistance":
        """How far ``generated`` is from ``source`` in the log-mel domain: the log-spectral distance (dB) and the
        mean absolute difference (nats) of their ``ops.logmel`` frames, per sequence (``ops.feature_distance``).
        Both are (B, T) integer class indices on the GPU, or (B, Q, T) one-hot.

        The frames are made with the settings of the model's ``local_conditioning`` record (a model trained with
        ``--use_mel 1``, or loaded from its checkpoint); any of ``n_fft``, ``hop``, ``n_mels``, ``rate``, ``f_min``,
        ``f_max`` given here takes the record's place, and a model without the record needs the first four.  A frame
        counts when its window lies wholly past the first ``skip`` samples (default: ``receptive_fields``, the prompt
        of a copy-synthesis, which is the source's own) and inside the row's ``lengths[b]`` real samples (default:
        the whole row) -- ``ops.distance_frame_span``.

        Under ``preemphasis`` both sides are the EMPHASISED signal, because that is what the class indices encode:
        the distance weighs high frequencies more than one taken on the de-emphasised audio would.

        Returns a ``SpectralDistance``: ``lsd_db``, ``l1`` (B,) float64, ``frames`` (B,) int32 and, on request,
        ``per_frame`` (B, F) float32 (else None).  A row with no counted frame has 0.0 in both."""
        from . import ops
        rec = getattr(self, "local_conditioning", None) or {}
        given = {"n_fft": n_fft, "hop": hop, "n_mels": n_mels, "rate": rate, "f_min": f_min, "f_max": f_max}
        keys = {"n_fft": "mel_fft", "hop": "local_hop", "n_mels": "local_channels", "rate": "audio_rate",
                "f_min": "mel_fmin", "f_max": "mel_fmax"}
        s = {k: (v if v is not None else rec.get(keys[k])) for k, v in given.items()}
        missing = [k for k in ("n_fft", "hop", "n_mels", "rate") if s[k] is None]
        if missing:
            raise ValueError("spectral_distance: the model has no local_conditioning record (it was not trained with "
                             "--use_mel 1); pass the keyword arguments n_fft, hop, n_mels, rate (and f_min, f_max) "
                             f"instead -- missing: {', '.join(missing)}")
        g, x = self._class_indices(generated, "generated"), self._class_indices(source, "source")
        if g.shape != x.shape or g.device != x.device:
            raise ValueError(f"generated {tuple(g.shape)} on {g.device} and source {tuple(x.shape)} on {x.device} "
                             "must agree")
        B, T = (int(v) for v in x.shape)
        skip = self.receptive_fields if skip is None else skip
        first, count = ops.distance_frame_span(lengths, T, int(s["n_fft"]), int(s["hop"]), skip, batch=B)
        if len(first) != B:
            raise ValueError(f"lengths names {len(first)} sequences, the batch holds {B}")
        F = ops.logmel_frames(T, int(s["hop"]))
        first = [min(f, F - n) for f, n in zip(first, count)]  # (an empty span past the last frame starts at F)
        fbank = ops.mel_filterbank(int(s["n_mels"]), int(s["n_fft"]), float(s["rate"]),
                                   0.0 if s["f_min"] is None else float(s["f_min"]), s["f_max"])
        mels = [ops.logmel(i, self.input_channels, int(s["n_fft"]), int(s["hop"]), fbank) for i in (g, x)]
        out = ops.feature_distance(mels[0], mels[1], first, count, per_frame=per_frame)
        return SpectralDistance(out["lsd_db"], out["l1"], out["frames"], out.get("per_frame"))

    @torch.no_grad()
    def pitch_distance(self, generated, source, lengths=None, skip: Optional[int] = None, *,
                       win: Optional[int] = None, hop: Optional[int] = None, rate: Optional[float] = None,
                       f_min: float = 60.0, f_max: float = 500.0, threshold: float = 0.15,
                       gross_ratio: float = 0.2) -> "PitchDistance":
        """How far the pitch of ``generated`` is from that of ``source``: both are tracked frame by frame with
        ``ops.pitch`` (YIN) and the two tracks compared with ``ops.pitch_distance``, per sequence.  Both are (B, T)
        integer class indices on the GPU, or (B, Q, T) one-hot -- the arguments of ``spectral_distance``, which this
        call mirrors.

        ``win`` (the samples a lag's difference is summed over), ``hop`` and ``rate`` come from the model's
        ``local_conditioning`` record -- ``mel_fft``, ``local_hop`` and ``audio_rate`` -- so the pitch frames are the
        log-mel frames; a keyword given here takes the record's place, and a model without the record needs all
        three.  The lags searched are ``ops.pitch_lags(rate, f_min, f_max)``.  A frame covers ``win + tau_max``
        samples and counts when they lie wholly past the first ``skip`` samples (default: ``receptive_fields``, the
        prompt of a copy-synthesis) and inside the row's ``lengths[b]`` real samples:
        ``ops.distance_frame_span`` with ``n_fft = win + tau_max``.

        Under ``preemphasis`` A > 0 both sides are tracked on the DE-EMPHASISED audio (``ops.deemphasis_pcm16`` of the
        classes, over 32768, as a float32 waveform), not on what the class indices encode as ``spectral_distance``
        does: pre-emphasis attenuates the fundamental, which is what a pitch tracker needs.  At A = 0 the class
        indices go to the tracker as they are.

        Returns a ``PitchDistance``: ``f0_rmse_cents`` (B,) float64 -- the RMS of 1200 log2(F0 generated / F0 source)
        over the frames voiced in both, 0.0 where there are none --, ``voiced_frames``, ``vuv_errors`` (voiced in
        exactly one), ``gross_errors`` (periods more than ``gross_ratio`` apart) and ``frames``, (B,) int32 each."""
        from . import ops
        rec = getattr(self, "local_conditioning", None) or {}
        given = {"win": win, "hop": hop, "rate": rate}
        keys = {"win": "mel_fft", "hop": "local_hop", "rate": "audio_rate"}
        s = {k: (v if v is not None else rec.get(keys[k])) for k, v in given.items()}
        missing = [k for k in ("win", "hop", "rate") if s[k] is None]
        if missing:
            raise ValueError("pitch_distance: the model has no local_conditioning record (it was not trained with "
                             "--use_mel 1); pass the keyword arguments win, hop and rate instead -- missing: "
                             f"{', '.join(missing)}")
        tau_min, tau_max = ops.pitch_lags(float(s["rate"]), f_min, f_max)
        win, hop, tau_min, tau_max, threshold = ops.check_pitch_settings(int(s["win"]), int(s["hop"]), tau_min,
                                                                         tau_max, threshold)
        g, x = self._class_indices(generated, "generated"), self._class_indices(source, "source")
        if g.shape != x.shape or g.device != x.device:
            raise ValueError(f"generated {tuple(g.shape)} on {g.device} and source {tuple(x.shape)} on {x.device} "
                             "must agree")
        B, T = (int(v) for v in x.shape)
        skip = self.receptive_fields if skip is None else skip
        first, count = ops.distance_frame_span(lengths, T, win + tau_max, hop, skip, batch=B)
        if len(first) != B:
            raise ValueError(f"lengths names {len(first)} sequences, the batch holds {B}")
        F = ops.logmel_frames(T, hop)
        first = [min(f, F - n) for f, n in zip(first, count)]  # (an empty span past the last frame starts at F)
        a = self.preemphasis
        settings = dict(win=win, hop=hop, tau_min=tau_min, tau_max=tau_max, threshold=threshold)
        tracks = [ops.pitch_of_classes(i, self.input_channels, a, **settings) for i in (g, x)]
        out = ops.pitch_distance(tracks[0]["period"], tracks[1]["period"], first, count, gross_ratio=gross_ratio)
        return PitchDistance(out["f0_rmse_cents"], out["voiced_frames"], out["vuv_errors"], out["gross_errors"],
                             out["frames"])

    @torch.no_grad()
    def classify(self, audio, video=None, log_prior=None, logits_budget_bytes: int = 1 << 30, lengths=None, *,
                 local_features=None):
        """Which class label explains ``audio`` best (a model built with ``global_classes = G > 0``; ValueError
        otherwise): returns ``(loglik, posterior)``, both (B, G) -- ``loglik[b, c]`` = log p(x_b | class c), the
        ``-nll`` of ``score`` with ``global_features = c``, and ``posterior`` = softmax(loglik + ``log_prior``)
        over the classes (``log_prior``: (G,) or (B, G); default uniform).

        The (class, sequence) pairs run through the scoring pass of ``score`` in chunks of as many pairs as keep a
        chunk's logits within ``logits_budget_bytes`` (default 1 GiB; at least one pair), the audio's indices and
        the up-sampled video formed once; each chunk takes the label path ``score`` would take for its batch.
        ``lengths``: as in ``score`` -- each sequence's likelihood runs over its own real samples."""
        from .ops import score_indices
        G = int(self.global_classes)
        if G <= 0:
            raise ValueError("classify needs a model built with global_classes (there are no labels to tell apart)")
        if isinstance(logits_budget_bytes, bool) or not isinstance(logits_budget_bytes, int) or logits_budget_bytes < 1:
            raise ValueError(f"logits_budget_bytes must be a positive integer, got {logits_budget_bytes!r}")
        B = int(audio.shape[0])
        if log_prior is not None:
            log_prior = torch.as_tensor(log_prior)
            if tuple(log_prior.shape) not in ((G,), (B, G)):
                raise ValueError(f"log_prior must be ({G},) or ({B}, {G}), got {tuple(log_prior.shape)}")
        self._lengths_checks(lengths, video)
        _, mode = self._score_checks(audio, video, torch.zeros(B, dtype=torch.int64), local_features)
        valid = self._valid_on_device(lengths, audio)
        context = self._context_of(audio, video, local_features)
        idx = self._indices_of(audio)  # ValueError unless one-hot
        positions = int(audio.shape[2]) - self.receptive_fields
        per_pair = 4 * self.input_channels * max(positions, 1)
        step = max(1, logits_budget_bytes // per_pair)
        pairs = torch.arange(G * B, device=idx.device)  # class-major: pair = c B + b
        E = self.global_embedding.weight.detach()
        nll = []
        for p0 in range(0, G * B, step):
            rows = pairs[p0:p0 + step]
            seq, cls = rows % B, rows // B
            raw = score_indices(self, idx[seq], None if context is None else context[seq], E[cls], 1.0, False, False,
                                mode, valid=None if valid is None else valid[seq])
            nll.append(raw["seq_nll"])
        loglik = -torch.cat(nll).view(G, B).t().contiguous()
        post = loglik.double() if log_prior is None else loglik.double() + log_prior.to(loglik.device).double()
        return loglik, torch.softmax(post, dim=1).to(torch.float32)

    def _generate_setup(self, audio, video, global_features, n_samples, temperature, what: str = "generate",
                        windowed: bool = False):
        """What ``generate()`` and ``generate_stream()`` share, up to the launch plan: the checks in their order, the
        settings taken from the attributes, the context, the prompt's class indices, the seed and the plan of
        ``auto_plan``.  Returns a namespace -- ``idx``, ``rf``, ``n_total``, and ``make`` = None where there is nothing to
        generate, else ``make(variant, group)`` (a new generator, not yet primed), ``variant`` / ``group`` (0: one
        launch) of the plan and ``fallback()``: the kernel a timed-out pipelined call is rerun on -- recorded in
        ``last_generate_fallback`` and announced on stderr.  ``windowed`` (``generate_stream(context="windowed")``): the
        generators take a ``ContextSource`` -- the frame-rate projection and / or the label's vectors -- in place of the
        (B, C, n_total) context; the fallback's generator is built from the same source."""
        from types import SimpleNamespace
        from .ops import global_vector
        local_features, self._gen_local_features = self.generate_local_features, None  # (taken: one call uses it)
        self._local_checks(audio, video, local_features,
                           n_total=max(int(audio.shape[2]) if n_samples is None else int(n_samples), 1))
        gvec = global_vector(self, global_features, int(audio.shape[0]))
        top_k, top_p, seed = self.generate_top_k, self.generate_top_p, self.generate_seed
        guidance = self.generate_guidance
        if N.any_per_sequence(guidance) or guidance != 1.0:  # (1.0: today's path, untouched)
            guidance = N.guidance_scales(int(audio.shape[0]), guidance)  # ValueError for a wrong length
            if gvec is None:
                raise ValueError("generate_guidance needs a model built with global_classes")
        else:
            guidance = None
        per_seq = N.any_per_sequence(temperature, seed)
        if per_seq:  # (validates lengths and values; the seed drawn below replaces the placeholder)
            N.seq_sampling_array(int(audio.shape[0]), self.input_channels, temperature, top_k, top_p,
                                 0 if seed is None else seed)
        else:
            temperature = float(temperature)
        self.eval()  # the reference leaves the module in eval mode
        # BUILD DEFINITION for video != None (the reference fails its size assert there,
        # SURVEY.md Q7): the context column of time t conditions the step that consumes x_t
        rf = self.receptive_fields
        n_total = int(audio.shape[2]) if n_samples is None else int(n_samples)
        source = None
        if windowed and (local_features is not None or gvec is not None):
            from .generation import ContextSource
            from .ops import project_features, upsample_features
            glob = None if gvec is None else gvec.detach().to(torch.float32).contiguous()
            if local_features is None:
                source = ContextSource(glob=glob)
            else:
                source = ContextSource(project_features(self, local_features), int(self.local_hop), glob,
                                       prompt=lambda P: upsample_features(self, local_features, P))
        context = None if windowed else self._context_of(audio, video, local_features, n_total=max(n_total, 1))
        idx = self._indices_of(audio)
        plan = SimpleNamespace(idx=idx, rf=rf, n_total=n_total, make=None)
        if idx.shape[1] < rf or n_total <= rf:
            return plan
        if seed is None:
            seed = int(torch.empty((), dtype=torch.int64).random_().item())
        state = self._decoder_state()
        if context is None and gvec is None and source is None:
            state = {k: v for k, v in state.items() if ".context_conv_" not in k}
        elif context is not None and context.shape[2] < n_total:
            raise ValueError(f"the upsampled video covers {context.shape[2]} samples, "
                             f"n_samples={n_total} asked for")
        kw = dict(batch=idx.shape[0], n_total=n_total, device=audio.device,
                  temperature=temperature, seed=seed, context=context,
                  global_context=None if gvec is None else gvec.detach().to(torch.float32).contiguous(),
                  sampling=self.generate_sampling, top_k=top_k, top_p=top_p)
        if guidance is not None:
            kw["guidance"] = guidance
        if source is not None:
            kw.update(context=None, global_context=None, context_source=source)

        def make(variant, group):
            if group:
                return GroupedGenerator(self.layer_size, self.stack_size, self.input_channels,
                                        self.residual_channels, self.skip_channels, state,
                                        group=group, variant=variant, **kw)
            return RingGenerator(self.layer_size, self.stack_size, self.input_channels,
                                 self.residual_channels, self.skip_channels, state,
                                 variant=variant, **kw)

        with torch.cuda.device(audio.device):
            if self._gen_variant == N.GEN_AUTO:
                kind, group, variant = auto_plan(self._dims, idx.shape[0],
                                                 context is not None or gvec is not None or source is not None,
                                                 guided=guidance is not None)
            else:
                kind, group, variant = "single", 0, self._gen_variant
                if variant == N.GEN_PIPE_F16 and idx.shape[0] > max_pipe_batch(self._dims, variant,
                                                                               guided=guidance is not None):
                    kind, group = "grouped", max_pipe_batch(self._dims, variant, guided=guidance is not None)  # groups take turns

        def fallback():
            # the pipelined kernel needs all its stages co-resident and something else held
            # CUs: rerun THIS call (same prompt, same seed) on a kernel without hand-offs
            with torch.cuda.device(audio.device):
                lib = N.lib()
                # (STREAM: C = K = 64, any batch in one launch, conditioned or not -- r4; GENERIC otherwise)
                fb = N.GEN_STREAM if guidance is None and lib.mvn_gen_variant(
                    self._dims, N.GEN_STREAM, idx.shape[0]) == N.GEN_STREAM else N.GEN_GENERIC  # (guided: GENERIC)
            self.last_generate_fallback = fb
            name = {N.GEN_STREAM: "STREAM", N.GEN_GENERIC: "GENERIC"}[fb]
            print(f"[movenet_amd] {what}: pipelined kernel (variant {variant}) timed out waiting for a "
                  f"co-resident stage; rerunning this call on {name}"
                  + (" -- fp32 arithmetic instead of the fp16 operands asked for" if variant == N.GEN_PIPE_F16
                     else ""), file=sys.stderr, flush=True)
            return fb

        plan.make, plan.variant, plan.group, plan.fallback = make, variant, group if kind == "grouped" else 0, fallback
        return plan

    @torch.no_grad()
    def generate(self, audio, video=None, global_features=None, n_samples: Optional[int] = None,
                 temperature=1.0):
        """wavenet.py:193-239: copy the first RF prompt samples, then generate
        autoregressively up to n_samples (default: the prompt's own length).

        ``temperature`` takes one value or a sequence of B values, one per sequence of the batch (a temperature sweep
        on one prompt is ONE launch: repeat the prompt), and ``generate_seed`` likewise; with either a sequence,
        sequence b draws on its own seed and row b whatever the launch plan.  A wrong length or a bad value is a
        ValueError before anything runs.  ``global_features``: as in ``forward`` -- the label's vector conditions
        every step (required for a model built with ``global_classes``).  A model built with ``local_channels`` reads
        its feature frames from ``generate_local_features`` (the signature stays the reference's, as for the other
        generation settings; this one is used up by the call): frames for all ``n_samples`` -- the up-sampled (B, C, n_samples) tensor is the
        generators' ``context``."""
        plan = self._generate_setup(audio, video, global_features, n_samples, temperature)
        idx, rf, n_total = plan.idx, plan.rf, plan.n_total
        if plan.make is None:
            # nothing to generate: the reference returns zeros with the prompt copied in
            out = torch.zeros(audio.shape[0], audio.shape[1], n_total, dtype=audio.dtype,
                              device=audio.device)
            n = min(rf, n_total, audio.shape[2])
            out[:, :, :n] = audio[:, :, :n]
            return out

        def run(variant, group):
            gen = plan.make(variant, group)
            gen.prime(idx[:, :rf])
            gen.advance(n_total - rf)
            gen.check_errors()  # synchronises; never hand unchecked samples on
            return gen

        try:
            gen = run(plan.variant, plan.group)
        except PipeHandoffTimeout:
            gen = run(plan.fallback(), 0)
        return self._one_hot_of(gen.samples, audio.dtype)

    @torch.no_grad()
    def generate_stream(self, audio, video=None, global_features=None, n_samples: Optional[int] = None,
                        temperature=1.0, chunk: int = 4000, context: str = "whole"):
        """``generate()`` handing the audio out while it is being made: a generator of ``(t0, pcm)`` --
        ``pcm`` a (B, n) int16 numpy array on the host, the 16-bit PCM of columns [t0, t0 + n) of every sequence, to the
        bit what ``callbacks.write_wav`` stores for ``ops.mu_law_decode`` of ``generate()``'s classes under the same
        settings and ``generate_seed``.  First ``(0, pcm)`` of the copied prompt columns [0, RF), then one pair per
        launch of ``chunk`` steps (the last may be shorter); an array is valid until the next ``next()``.  Where
        ``generate()`` has nothing to generate, the one pair is its zeros-plus-prompt result: all ``n_samples`` columns,
        class 0 behind the prompt.

        Same arguments, attributes, checks (in the same order, at the first ``next()``) and launch plan as
        ``generate()``; ``chunk < 1`` is a ValueError before any of them.  A hand-off timeout of a pipelined kernel
        before the first generated chunk has been handed out reruns the call on the fallback kernel, as ``generate()``
        does; later it reaches the caller as ``PipeHandoffTimeout`` -- audio already delivered cannot be taken back.

        ``context``: "whole" builds the (B, C, n_samples) conditioning and its time-major copy before the
        first step, as ``generate()`` does; "windowed" keeps the frame-rate projection of the feature frames and / or
        the label's vectors and forms each launch's columns in front of it, in one buffer of B x chunk x C floats -- the
        same PCM byte for byte, in memory that does not grow with ``n_samples``.  Not with ``video`` (ValueError: clips
        are capped at MAX_AUDIO_FRAMES, and the transposed-conv up-sampler has no windowed form); on a model with neither
        labels nor local features it is the unconditioned path."""
        from .generation import plan_chunks
        from .ops import pcm16_chunk
        plan_chunks(0, 0, chunk)  # ValueError before anything is used up
        if context not in ("whole", "windowed"):
            raise ValueError(f"context must be 'whole' or 'windowed', got {context!r}")
        if context == "windowed" and video is not None:
            raise ValueError("context='windowed' cannot be combined with video: the video up-sampler has no windowed form")
        plan = self._generate_setup(audio, video, global_features, n_samples, temperature, what="generate_stream",
                                    windowed=context == "windowed")
        idx, rf, n_total = plan.idx, plan.rf, plan.n_total
        # (preemphasis > 0: one filter state per call, zero before column 0; the prompt's columns go through it first)
        a = self.preemphasis
        filt = {} if a <= 0.0 else {"deemphasis": a, "state": torch.zeros(idx.shape[0], dtype=torch.float64,
                                                                          device=idx.device)}
        if plan.make is None:
            n = min(rf, n_total, int(audio.shape[2]))
            given = torch.zeros(idx.shape[0], max(n_total, 0), dtype=torch.int32, device=idx.device)
            given[:, :n] = idx[:, :n]
            yield 0, pcm16_chunk(given, 0, given.shape[1], self.input_channels, **filt).cpu().numpy()
            return
        yield 0, pcm16_chunk(idx, 0, rf, self.input_channels, **filt).cpu().numpy()

        def chunks_of(variant, group):
            gen = plan.make(variant, group)
            gen.prime(idx[:, :rf])
            # (a rerun on the fallback kernel starts again behind the prompt: each run filters from a copy of that state)
            return gen.stream(n_total - rf, chunk, **(filt and {"deemphasis": a, "state": filt["state"].clone()}))

        chunks = chunks_of(plan.variant, plan.group)
        try:
            first = next(chunks, None)
        except PipeHandoffTimeout:
            chunks = chunks_of(plan.fallback(), 0)
            first = next(chunks, None)
        if first is not None:
            yield first
            yield from chunks
