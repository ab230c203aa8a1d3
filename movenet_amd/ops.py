"""Full-sequence forward/backward through the C ABI, wrapped as one
``torch.autograd.Function`` so that ``WaveNet.forward`` is trainable with the
stock torch optimizers (/root/reference/movenet/wavenet.py:158-191 and the
autograd graph PyTorch would build for it).

torch is used for device memory (activation buffers come from the caching
allocator) and for the autograd hook; every arithmetic kernel is HIP.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Tuple

import ctypes
import os

import torch

from . import _native as N
from .generation import _require_gpu, _stream_ptr, pack_params

C_void3 = ctypes.c_void_p * 3

_LAYER_PARAMS = ("conv_filter.conv.weight", "conv_gate.conv.weight", "conv_residual.weight",
                 "conv_residual.bias", "conv_skip.weight", "conv_skip.bias")
_CTX_PARAMS = ("context_conv_filter.weight", "context_conv_filter.bias",
               "context_conv_gate.weight", "context_conv_gate.bias")
VIDEO_PARAMS = ("video_conv.weight", "video_conv.bias",
                "video_transpose.0.weight", "video_transpose.0.bias",
                "video_transpose.1.weight", "video_transpose.1.bias",
                "video_transpose.2.weight", "video_transpose.2.bias")


def decoder_param_names(n_layers: int, with_context: bool = False) -> List[str]:
    """Parameters the decoder uses, in the order they are passed to autograd."""
    per_layer = _LAYER_PARAMS + (_CTX_PARAMS if with_context else ())
    names = ["causal_conv.conv.weight"]
    for l in range(n_layers):
        names += [f"residual_conv_stack.conv_layers.{l}.{p}" for p in per_layer]
    names += ["dense_conv.conv1.weight", "dense_conv.conv1.bias",
              "dense_conv.conv2.weight", "dense_conv.conv2.bias"]
    return names


class VideoGradSlot:
    """Hand-over between the two autograd nodes of a conditioned step.  The decoder's backward
    (which runs first: it produces the context gradient) allocates ONE zero-filled flat buffer
    for its own gradients AND the eight video-encoder gradients behind them, in the order
    ``optim.order_like_backward(model, with_context=True)`` lays the parameters out; the
    up-sampler's backward then writes into those views instead of eight buffers of its own.
    One storage => one all-reduce message (parallel.contiguous_grad_span) and one AdamW launch."""

    def __init__(self, shapes):
        self.shapes = [tuple(s) for s in shapes]
        self.sizes = [int(torch.Size(s).numel()) for s in self.shapes]
        self.total = sum(self.sizes)
        self.views = None

    def carve(self, tail: torch.Tensor) -> None:
        views, off = [], 0
        for shape, k in zip(self.shapes, self.sizes):
            views.append(tail[off:off + k].view(shape))
            off += k
        self.views = views

    def take(self):
        views, self.views = self.views, None
        return views


class ForwardBuffers:
    """Device buffers of one forward pass (sizes: include/movenet_hip.h)."""

    def __init__(self, dims: N.Dims, batch: int, t_len: int, save: bool, device, ctx=None,
                 dense=None):
        lib = N.lib()
        L = dims.layer_size * dims.stack_size
        C, K, Q = dims.residual_channels, dims.skip_channels, dims.input_channels
        S = N.check(lib.mvn_output_size(dims, t_len), "mvn_output_size")
        self.S, self.Tp, self.Sp = S, lib.mvn_padded_len(t_len), lib.mvn_padded_len(S + 31)
        f32 = dict(dtype=torch.float32, device=device)
        # (MOVENET_DEBUG_GUARD=1: a band of sentinels behind every buffer, checked after mvn_forward)
        self.guard = _GuardBands(device) if os.environ.get("MOVENET_DEBUG_GUARD") == "1" else None
        if self.guard is not None:
            lib.mvn_reload_switches()  # (debug / test mode: the MOVENET_HIP_* A/B switches may change inside the process)
        alloc = torch.empty if self.guard is None else self.guard.empty
        self.acts = alloc(((L + 1) if save else 2, batch, C, self.Tp), **f32)
        self.th = alloc((L, batch, C, self.Tp), **f32) if save else None
        self.sg = alloc((L, batch, C, self.Tp), **f32) if save else None
        self.z = alloc((batch, C, self.Tp), **f32)
        self.skip = alloc((batch, K, self.Sp), **f32)
        self.a1 = alloc((batch, Q, self.Sp), **f32)
        self.ctx = ctx
        self.struct = N.FwdBuffers(
            self.acts.data_ptr(), self.th.data_ptr() if save else None,
            self.sg.data_ptr() if save else None, self.z.data_ptr(), self.skip.data_ptr(),
            self.a1.data_ptr(), None if ctx is None else ctx.data_ptr(),
            0 if ctx is None else ctx.stride(1),
            None if dense is None else dense.data_ptr(), 0 if dense is None else dense.stride(1))
        self.dense = dense


class SequenceMode(NamedTuple):
    """What one full-sequence pass runs, decided once (plan_sequence, place_sequence); sequence_entry names its kernels."""
    precision: str = "fp32"         # operands of the layers' products: "fp32" / "fp16" / "bf16"
    conditioning: str = "none"      # what reaches the kernels: "none" / "context" (B, C, T) / "bias" (B, C) vectors
    label_in_context: bool = False  # a label's vector has joined the context (general path of global conditioning)
    loss_rule: int = N.LOSS_REFERENCE
    grad_mode: bool = True          # grad mode at the call (it is off inside an autograd Function's forward)
    video_slot: object = None       # VideoGradSlot of the context's up-sampler node, or None


class SequenceEntry(NamedTuple):
    forward: str
    backward: Optional[str]              # None: inference only
    path_query: Optional[str] = None     # asked before the pass is placed (place_sequence); None: any shape runs
    scratch_query: Optional[str] = None  # floats of the backward's caller-owned scratch; None: it takes none
    rowsum: bool = False                 # the backward fills (L, B, 128) row sums for mvn_global_bias_backward


# Every legal (precision, conditioning) and the entry points that run it.  "bias" rows run mvn_global_bias in front of
# the forward and mvn_global_bias_backward behind the backward.  "context+label": fp32, C = K = 64, a label in the
# context -- the one-kernel layer backward with a scratch of its own (dlogit / da1, where it looks otherwise, do not
# hold it at short outputs or small Q).  (mvn_bf16_ctx_path is not asked: the entry points refuse for themselves.)
SEQUENCE_ENTRIES = {
    ("fp32", "none"): SequenceEntry("mvn_forward", "mvn_backward"),
    ("fp32", "context"): SequenceEntry("mvn_forward", "mvn_backward"),
    ("fp32", "context+label"): SequenceEntry("mvn_forward", "mvn_backward_scratch", scratch_query="mvn_global_scratch_floats"),
    ("fp32", "bias"): SequenceEntry("mvn_forward_global", "mvn_backward_global", "mvn_global_fast_path",
                                    "mvn_global_scratch_floats", True),
    ("fp16", "none"): SequenceEntry("mvn_forward_f16", None),
    ("fp16", "context"): SequenceEntry("mvn_forward_f16", None),
    ("bf16", "none"): SequenceEntry("mvn_forward_bf16", "mvn_backward_bf16"),
    ("bf16", "bias"): SequenceEntry("mvn_forward_bf16_global", "mvn_backward_bf16_global", "mvn_global_bf16_path",
                                    "mvn_global_bf16_scratch_floats", True),
    ("bf16", "context"): SequenceEntry("mvn_forward_bf16_ctx", "mvn_backward_bf16_ctx", scratch_query="mvn_bf16_ctx_scratch_floats"),
}


def sequence_entry(mode: SequenceMode, dims) -> SequenceEntry:
    """The row of SEQUENCE_ENTRIES that runs ``mode``; ValueError, by name, for a combination that has none."""
    cond = mode.conditioning
    if (mode.precision == "fp32" and cond == "context" and mode.label_in_context
            and dims.residual_channels == 64 and dims.skip_channels == 64):
        cond = "context+label"
    entry = SEQUENCE_ENTRIES.get((mode.precision, cond))
    if entry is None:
        raise ValueError(f"movenet_amd: no sequence kernels run precision {mode.precision!r} with conditioning {cond!r}")
    return entry


def run_forward(dims: N.Dims, sd: Dict[str, torch.Tensor], idx: torch.Tensor, normalize: bool,
                remove_last: bool, save: bool, mode: SequenceMode = SequenceMode(),
                cond=None) -> Tuple[torch.Tensor, ForwardBuffers]:
    """idx: (B,T) int32 class indices, or a (B,Q,T) fp32 tensor for inputs that are
    not one-hot (dense causal conv).  ``mode`` picks the entry point (SEQUENCE_ENTRIES); ``cond`` is what
    ``mode.conditioning`` names: the (B, C, T) context, the (B, C) fp32 global vectors of the one-vector-per-layer path
    (C = K = 64; the caller has asked the entry's path query), or None."""
    lib = N.lib()
    entry = sequence_entry(mode, dims)
    assert (cond is None) == (mode.conditioning == "none"), "mode.conditioning and the tensor given for it disagree"
    ctx, gvec = (cond, None) if mode.conditioning == "context" else (None, cond)
    _require_gpu(idx, "audio")
    dense = None
    if idx.dim() == 3:
        dense = idx.detach().to(torch.float32).contiguous()
        B, _, T = dense.shape
    else:
        B, T = idx.shape
    L = dims.layer_size * dims.stack_size
    dev = idx.device
    if ctx is not None:
        # same check as the reference's assert (wavenet.py:170-174)
        assert tuple(ctx.shape) == (B, dims.residual_channels, T), (
            "expected video and audio tensors to have equal sizes, found "
            f"{tuple(ctx.shape)}, {(B, dims.residual_channels, T)}")
        ctx = ctx.detach().to(torch.float32).contiguous()
    with torch.cuda.device(dev):
        buf = ForwardBuffers(dims, B, T, save, dev, ctx, dense)
        s_out = buf.S - (1 if remove_last else 0)
        out = (torch.empty if buf.guard is None else buf.guard.empty)(
            (B, dims.input_channels, max(s_out, 0)), dtype=torch.float32, device=dev)
        params, keep = pack_params(dims, sd, L)
        name, tail = entry.forward, ()
        if gvec is not None:  # one 2C-vector per (layer, sequence) instead of a context product per column
            gbias = (torch.empty if buf.guard is None else buf.guard.empty)((L, B, 128), dtype=torch.float32, device=dev)
            N.check(lib.mvn_global_bias(dims, params, gvec.data_ptr(), B, gbias.data_ptr(), _stream_ptr(dev)),
                    "mvn_global_bias")
            tail = (gbias.data_ptr(),)
            buf.gbias = gbias
        N.check(getattr(lib, name)(dims, params, None if dense is not None else idx.data_ptr(),
                                   0 if dense is not None else idx.stride(0), B, T, buf.struct,
                                   out.data_ptr(), int(normalize), int(remove_last), int(save), *tail,
                                   _stream_ptr(dev)), name)
        if buf.guard is not None:
            buf.guard.check("mvn_forward")
    buf._keep = keep  # parameter tensors stay alive until the kernels have run
    return out, buf


class _WaveNetFunction(torch.autograd.Function):
    """args: mode (SequenceMode), dims, names, idx, normalize, remove_last, ctx (Tensor or None), gvec (Tensor or
    None), *params.  ``gvec``: the (B, C) global vectors of ``mode.conditioning == "bias"`` (``context`` is None then)."""
    N_FIXED = 8

    @staticmethod
    def forward(ctx_, mode, dims, names, idx, normalize, remove_last, context, gvec, *params):
        sd = dict(zip(names, params))
        # (grad mode itself is off inside forward(): the caller records whether it was on)
        save = any(ctx_.needs_input_grad[6:]) and mode.grad_mode
        if save and sequence_entry(mode, dims).backward is None:
            raise RuntimeError("movenet_amd: forward_precision 'fp16' is inference-only "
                               "(mvn_backward differentiates the fp32 forward); use torch.no_grad()")
        gvec = None if gvec is None else gvec.detach().to(torch.float32).contiguous()
        out, buf = run_forward(dims, sd, idx, normalize, remove_last, save, mode, context if gvec is None else gvec)
        ctx_.mode, ctx_.dims, ctx_.names, ctx_.idx, ctx_.buf, ctx_.gvec = mode, dims, names, idx, buf, gvec
        ctx_.normalize, ctx_.remove_last, ctx_.saved_fwd = normalize, remove_last, save
        ctx_.has_context = context is not None
        ctx_.save_for_backward(out, *params)
        return out

    @staticmethod
    def backward(ctx_, dout):
        out, *params = ctx_.saved_tensors
        dout = dout.to(torch.float32).contiguous()
        grads, dctx, dgvec = _run_backward(ctx_, params, out, dout, None)
        return _grads_for_autograd(ctx_, grads, dctx, dgvec, _WaveNetFunction.N_FIXED, ctx_.needs_input_grad)


class _GuardBands:
    """Debug allocator (MOVENET_DEBUG_GUARD=1): tensors with a band of sentinel values behind them; ``check``
    raises if a kernel wrote past the end of one (r3: the fused backward halves' bias partial sums did, for short
    sequences in small batches -- into whichever tensor the allocator had placed next)."""
    BAND, SENTINEL = 1 << 18, -1234.5   # 1 MiB of floats behind each tensor

    def __init__(self, device):
        self.device, self.bands = device, []

    def empty(self, shape, dtype=torch.float32, device=None):
        n = 1
        for k in shape:
            n *= int(k)
        raw = torch.empty(n + self.BAND, dtype=dtype, device=self.device)
        raw[n:].fill_(self.SENTINEL)
        self.bands.append((tuple(shape), raw[n:]))
        return raw[:n].view(shape)

    def check(self, what: str) -> None:
        for shape, band in self.bands:
            bad = int((band != self.SENTINEL).sum().item())
            if bad:
                raise RuntimeError(f"movenet_amd: {what} wrote {bad} floats past the end of a {shape} scratch tensor")


def _run_backward(ctx_, params, out, dout, fill_dlogit):
    """mvn_backward for a saved forward.  ``dout``: gradient w.r.t. the model output, or None
    when ``fill_dlogit(dlogit, Sp, pad)`` writes the gradient w.r.t. the logits itself (the
    fused loss).  Returns ({name: grad view into ONE flat buffer}, dctx or None, dgvec or None)."""
    if not ctx_.saved_fwd:
        raise RuntimeError("movenet_amd: forward ran without saved activations")
    lib = N.lib()
    dims, names, idx, buf = ctx_.dims, ctx_.names, ctx_.idx, ctx_.buf
    L = dims.layer_size * dims.stack_size
    C, K, Q = dims.residual_channels, dims.skip_channels, dims.input_channels
    dense_in = idx.dim() == 3
    B, T = (idx.shape[0], idx.shape[2]) if dense_in else idx.shape
    dev = idx.device
    sd = dict(zip(names, params))
    with torch.cuda.device(dev):
        # one zero-filled flat buffer, the per-parameter gradients are views into it (one
        # fill kernel instead of ~190; FlatGradSync all-reduces the buffer in place and
        # FlatAdamW steps over it with one kernel)
        sizes = [p.numel() for p in params]
        slot = ctx_.mode.video_slot if ctx_.has_context else None
        flat = torch.zeros(sum(sizes) + (slot.total if slot is not None else 0), dtype=torch.float32,
                           device=dev)
        if slot is not None:  # the video encoder's gradients live behind the decoder's
            slot.carve(flat[sum(sizes):])
        grads, off = {}, 0
        for n, p_, k in zip(names, params, sizes):
            grads[n] = flat[off:off + k].view(p_.shape)
            off += k
        gp, gkeep = pack_params(dims, grads, L)
        g = N.ParamGrads(gp.causal_w, gp.filter_w, gp.gate_w, gp.residual_w, gp.residual_b,
                         gp.skip_w, gp.skip_b, gp.head1_w, gp.head1_b, gp.head2_w, gp.head2_b,
                         gp.ctx_filter_w, gp.ctx_filter_b, gp.ctx_gate_w, gp.ctx_gate_b)
        f32 = dict(dtype=torch.float32, device=dev)
        # MOVENET_DEBUG_GUARD=1 (tests): every scratch tensor of the backward pass gets a guard band behind it,
        # checked after the call -- the library carves its slab / partial-sum scratch out of these tensors
        guard = _GuardBands(dev) if os.environ.get("MOVENET_DEBUG_GUARD") == "1" else None
        if guard is not None:
            lib.mvn_reload_switches()
        alloc = torch.empty if guard is None else guard.empty
        dx_a = alloc((B, C, buf.Tp), **f32)
        dx_b = alloc((B, C, buf.Tp), **f32)
        dfg = alloc((B, 2 * C, buf.Tp), **f32)
        dskip = alloc((B, K, buf.Sp), **f32)
        da1 = alloc((B, Q, buf.Sp), **f32)
        dlogit = alloc((B, Q, buf.Sp), **f32)
        dctx = alloc((B, C, buf.Tp), **f32) if ctx_.has_context else None
        bw = N.BwdBuffers(dx_a.data_ptr(), dx_b.data_ptr(), dfg.data_ptr(), dskip.data_ptr(),
                          da1.data_ptr(), dlogit.data_ptr(),
                          None if dctx is None else dctx.data_ptr())
        if fill_dlogit is not None:
            rf = N.check(lib.mvn_receptive_fields(dims), "mvn_receptive_fields")
            fill_dlogit(dlogit, buf.Sp, (rf - 1) & 31)
        params_c, pkeep = pack_params(dims, sd, L)
        # (a bf16 forward is differentiated by the bf16 backward: same operand rounding both ways)
        entry = sequence_entry(ctx_.mode, dims)
        name, gvec, tail, dgvec = entry.backward, ctx_.gvec, (), None
        if entry.scratch_query is not None:
            # the one-kernel layer backward's own scratch: slabs and partial sums, and (but bf16 + bias) the second pair
            # of scatter tensors -- the layer kernel leaves df | dg in the dfg tensor
            n_scratch = int(getattr(lib, entry.scratch_query)(dims, B, T))
            scratch = alloc((n_scratch,), **f32)
            tail = (scratch.data_ptr(), n_scratch)
        if entry.rowsum:
            # (row sums of df | dg: mvn_global_bias_backward turns them into the context-conv and the vectors' gradients)
            rowsum = alloc((L, B, 128), **f32)
            rowsum.zero_()
            tail += (rowsum.data_ptr(),)
        N.check(getattr(lib, name)(dims, params_c, g, None if dense_in else idx.data_ptr(),
                                   0 if dense_in else idx.stride(0), B, T,
                                   buf.struct, bw, None if out is None else out.data_ptr(),
                                   None if dout is None else dout.data_ptr(),
                                   int(ctx_.normalize), int(ctx_.remove_last), *tail, _stream_ptr(dev)),
                name)
        if entry.rowsum:
            dgvec = alloc((B, C), **f32)
            N.check(lib.mvn_global_bias_backward(dims, params_c, g, rowsum.data_ptr(), gvec.data_ptr(), B,
                                                 dgvec.data_ptr(), _stream_ptr(dev)), "mvn_global_bias_backward")
        if guard is not None:
            guard.check(name)
    # (buffers are released with the autograd node; a retained graph may run backward again)
    return grads, (dctx[:, :, :T] if dctx is not None else None), dgvec


def _grads_for_autograd(ctx_, grads, dctx, dgvec, n_fixed, need):
    dims, names = ctx_.dims, ctx_.names
    L = dims.layer_size * dims.stack_size
    last = f"residual_conv_stack.conv_layers.{L - 1}.conv_residual."
    result = []
    for n, want in zip(names, need[n_fixed:]):
        # the last layer's residual conv never reaches the output: the
        # reference leaves its .grad None, so do we
        result.append(None if (n.startswith(last) or not want) else grads[n])
    dcontext = dctx if (ctx_.has_context and need[n_fixed - 2]) else None
    return (*([None] * (n_fixed - 2)), dcontext, dgvec if need[n_fixed - 1] else None, *result)


def _checked_lengths(lengths, T: int):
    """``lengths`` of ``valid_columns`` as a host list of ints in [0, T], its ValueErrors included."""
    if isinstance(lengths, torch.Tensor):
        if lengths.dim() != 1 or lengths.is_floating_point() or lengths.is_complex() or lengths.dtype == torch.bool:
            raise ValueError(f"lengths must be a (batch,) integer tensor, got {tuple(lengths.shape)} {lengths.dtype}")
        if lengths.is_cuda:
            from .generation import HostWords
            words = lengths.detach().clamp(-1, 2 ** 31 - 1).to(torch.int32).contiguous()  # (a refused value stays one)
            tokens = [HostWords.publish(words[i:i + HostWords.MAXW]) for i in range(0, words.numel(), HostWords.MAXW)]
            values = [int(v) for t in tokens for v in HostWords.read(t)]
        else:
            values = lengths.tolist()
    else:
        if isinstance(lengths, (str, bytes)) or not hasattr(lengths, "__len__"):
            raise ValueError(f"lengths must be a sequence of one integer per sequence, got {lengths!r}")
        if getattr(lengths, "ndim", 1) != 1:
            raise ValueError(f"lengths must be one-dimensional, got shape {getattr(lengths, 'shape', None)}")
        values = lengths.tolist() if hasattr(lengths, "tolist") else list(lengths)
    for b, v in enumerate(values):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"lengths[{b}] = {v!r} is not an integer")
        if v < 0 or v > T:
            raise ValueError(f"lengths[{b}] = {v} lies outside [0, {T}]")
    return values


def valid_columns(lengths, T: int, RF: int):
    """Per-sequence count of loss columns from per-sequence lengths: ``valid_b = clamp(len_b - RF, 0, S)`` with
    ``S = T - RF`` (column s predicts sample RF + s, so it counts when that sample is real).  ``lengths``: (B,) host
    sequence, numpy array or integer tensor of ``0 <= len_b <= T``.  Returns a list of ints; ValueError -- before
    anything is launched -- for a wrong shape, a non-integer, a negative length or one above ``T``.  A tensor on the
    GPU is read once through the pinned word channel of the one-hot check (generation.HostWords)."""
    S = max(int(T) - int(RF), 0)
    return [min(max(v - int(RF), 0), S) for v in _checked_lengths(lengths, T)]


def _valid_for_batch(lengths, B: int, T: int, RF: int):
    """``lengths`` of a (B, ., T) batch -> host list of valid column counts (None stays None)."""
    if lengths is None:
        return None
    valid = valid_columns(lengths, T, RF)
    if len(valid) != B:
        raise ValueError(f"lengths names {len(valid)} sequences, the batch holds {B}")
    return valid


def counts_to_device(valid, device) -> torch.Tensor:
    """Host list of column counts -> (B,) int32 on ``device`` through pinned memory: the copy is asynchronous for
    the host (one from pageable memory is staged and may block it)."""
    with torch.cuda.device(device):
        return torch.tensor(valid, dtype=torch.int32).pin_memory().to(device, non_blocking=True)


class _WaveNetLossFunction(torch.autograd.Function):
    """Forward + the trainer's loss in one autograd node (row F3): the head's logits become
    probabilities and the loss / accuracy partial sums in ONE pass (mvn_softmax_ce_forward_ex);
    backward differentiates loss -> logits in ONE pass (mvn_softmax_ce_backward_ex) straight into
    mvn_backward's dlogit buffer.  args: mode (SequenceMode), dims, names, idx, target (B,S) int64, valid, ctx,
    gvec, *params; returns (loss, accuracy, probs).  ``valid``: None -- every column counts, the _ex calls -- or
    ``(counts, scale)``: (B,) int32 on the device and the host's 1 / max(sum of counts, 1), for the _len calls.  ``mode.loss_rule`` picks the loss: cross_entropy on the
    probabilities, or the negative log-likelihood of softmax(logits)."""
    N_FIXED = 8

    @staticmethod
    def forward(ctx_, mode, dims, names, idx, target, valid, context, gvec, *params):
        lib = N.lib()
        sd = dict(zip(names, params))
        save = any(ctx_.needs_input_grad[6:]) and mode.grad_mode
        # logits, last column dropped
        gvec = None if gvec is None else gvec.detach().to(torch.float32).contiguous()
        out, buf = run_forward(dims, sd, idx, False, True, save, mode, context if gvec is None else gvec)
        B, Q, S = out.shape
        if target.shape != (B, S):
            raise ValueError(f"target must be (batch, {S}), got {tuple(target.shape)}")
        tg = target.detach().to(device=out.device, dtype=torch.int64).contiguous()
        with torch.cuda.device(out.device):
            parts = max(lib.mvn_ce_parts(B, S), 1)
            loss_part = torch.zeros(parts, dtype=torch.float32, device=out.device)
            ok_part = torch.zeros(parts, dtype=torch.int32, device=out.device)
            if valid is None:
                N.check(lib.mvn_softmax_ce_forward_ex(out.data_ptr(), tg.data_ptr(), B, Q, S, loss_part.data_ptr(),
                                                      ok_part.data_ptr(), int(mode.loss_rule),
                                                      _stream_ptr(out.device)), "mvn_softmax_ce_forward_ex")
            else:
                if tuple(valid[0].shape) != (B,) or valid[0].dtype != torch.int32 or valid[0].device != out.device:
                    raise ValueError(f"valid counts must be ({B},) int32 on {out.device}")
                N.check(lib.mvn_softmax_ce_forward_len(out.data_ptr(), tg.data_ptr(), B, Q, S, loss_part.data_ptr(),
                                                       ok_part.data_ptr(), int(mode.loss_rule), valid[0].data_ptr(),
                                                       _stream_ptr(out.device)), "mvn_softmax_ce_forward_len")
        if valid is None:
            n = max(B * S, 1)
            loss = loss_part.sum() / n
            acc = ok_part.sum().to(torch.float32) / n
        else:
            loss = loss_part.sum() * valid[1]
            acc = ok_part.sum().to(torch.float32) * valid[1]
        ctx_.valid_scale = None if valid is None else valid[1]
        ctx_.mode, ctx_.dims, ctx_.names, ctx_.idx, ctx_.buf, ctx_.gvec = mode, dims, names, idx, buf, gvec
        ctx_.normalize, ctx_.remove_last, ctx_.saved_fwd = True, True, save
        ctx_.has_context = context is not None
        ctx_.save_for_backward(out, tg, *(() if valid is None else (valid[0],)), *params)
        ctx_.mark_non_differentiable(acc, out)
        return loss, acc, out

    @staticmethod
    def backward(ctx_, dloss, _dacc, _dprobs):
        lib = N.lib()
        probs, tg, *params = ctx_.saved_tensors
        counts = params.pop(0) if ctx_.valid_scale is not None else None
        B, Q, S = probs.shape
        up = dloss.detach().to(device=probs.device, dtype=torch.float32).reshape(1).contiguous()

        def fill(dlogit, Sp, pad):
            if counts is not None:
                N.check(lib.mvn_softmax_ce_backward_len(
                    probs.data_ptr(), tg.data_ptr(), B, Q, S, ctx_.valid_scale, up.data_ptr(), dlogit.data_ptr(), Q * Sp, Sp,
                    pad, S + 1, int(ctx_.mode.loss_rule), counts.data_ptr(), _stream_ptr(probs.device)),
                    "mvn_softmax_ce_backward_len")
                return
            N.check(lib.mvn_softmax_ce_backward_ex(
                probs.data_ptr(), tg.data_ptr(), B, Q, S, 1.0 / max(B * S, 1), up.data_ptr(),
                dlogit.data_ptr(), Q * Sp, Sp, pad, S + 1, int(ctx_.mode.loss_rule), _stream_ptr(probs.device)),
                "mvn_softmax_ce_backward_ex")

        grads, dctx, dgvec = _run_backward(ctx_, params, None, None, fill)
        return _grads_for_autograd(ctx_, grads, dctx, dgvec, _WaveNetLossFunction.N_FIXED, ctx_.needs_input_grad)


class _UpsampleVideoFunction(torch.autograd.Function):
    """video (B,F,64,64,Cin) -> context (B,C,1000F) through mvn_upsample_video."""

    @staticmethod
    def forward(ctx_, dims, slot, video, *params):
        lib = N.lib()
        _require_gpu(video, "video")
        if video.dim() != 5 or video.shape[2] != 64 or video.shape[3] != 64:
            raise ValueError(f"video must be (batch, frames, 64, 64, channels), got {tuple(video.shape)}")
        video = video.detach().to(torch.float32).contiguous()
        B, F, _, _, cin = video.shape
        C = dims.residual_channels
        dev = video.device
        pl = lib.mvn_padded_len
        with torch.cuda.device(dev):
            f32 = dict(dtype=torch.float32, device=dev)
            enc = torch.empty((B, C, pl(F)), **f32)
            u1 = torch.empty((B, C, pl(10 * F)), **f32)
            u2 = torch.empty((B, C, pl(100 * F)), **f32)
            out = torch.empty((B, C, 1000 * F), **f32)
            ps = [p.detach().to(torch.float32).contiguous() for p in params]
            vp = N.VideoParams(ps[0].data_ptr(), ps[1].data_ptr(),
                               (C_void3)(ps[2].data_ptr(), ps[4].data_ptr(), ps[6].data_ptr()),
                               (C_void3)(ps[3].data_ptr(), ps[5].data_ptr(), ps[7].data_ptr()))
            N.check(lib.mvn_upsample_video(dims, vp, video.data_ptr(), B, F, cin, enc.data_ptr(),
                                           u1.data_ptr(), u2.data_ptr(), out.data_ptr(),
                                           out.stride(1), _stream_ptr(dev)), "mvn_upsample_video")
        ctx_.dims, ctx_.shape, ctx_.slot = dims, (B, F, cin), slot
        ctx_.save_for_backward(video, enc, u1, u2, *ps)
        return out

    @staticmethod
    def backward(ctx_, dout):
        lib = N.lib()
        video, enc, u1, u2, *ps = ctx_.saved_tensors
        dims = ctx_.dims
        B, F, cin = ctx_.shape
        dev = video.device
        dout = dout.to(torch.float32).contiguous()
        with torch.cuda.device(dev):
            # zero-filled views behind the decoder's gradients when its backward has run (the
            # usual case: it produced dout), else eight buffers of this node's own
            grads = ctx_.slot.take() if ctx_.slot is not None else None
            if grads is None or grads[0].device != dev:
                grads = [torch.zeros_like(p) for p in ps]
            vp = N.VideoParams(ps[0].data_ptr(), ps[1].data_ptr(),
                               (C_void3)(ps[2].data_ptr(), ps[4].data_ptr(), ps[6].data_ptr()),
                               (C_void3)(ps[3].data_ptr(), ps[5].data_ptr(), ps[7].data_ptr()))
            vg = N.VideoParams(grads[0].data_ptr(), grads[1].data_ptr(),
                               (C_void3)(grads[2].data_ptr(), grads[4].data_ptr(), grads[6].data_ptr()),
                               (C_void3)(grads[3].data_ptr(), grads[5].data_ptr(), grads[7].data_ptr()))
            d_u2, d_u1, d_enc = torch.empty_like(u2), torch.empty_like(u1), torch.empty_like(enc)
            n_scratch = int(lib.mvn_upsample_video_scratch_floats(dims, B, F))  # per-workgroup weight-gradient slabs
            scratch = torch.empty(max(n_scratch, 1), dtype=torch.float32, device=dev)
            N.check(lib.mvn_upsample_video_backward(
                dims, vp, vg, video.data_ptr(), B, F, cin, enc.data_ptr(), u1.data_ptr(),
                u2.data_ptr(), dout.data_ptr(), dout.stride(1), d_u2.data_ptr(), d_u1.data_ptr(),
                d_enc.data_ptr(), scratch.data_ptr(), n_scratch, _stream_ptr(dev)), "mvn_upsample_video_backward")
        need = ctx_.needs_input_grad[3:]
        return (None, None, None, *[g if w else None for g, w in zip(grads, need)])


def upsample_video(model, video: torch.Tensor) -> torch.Tensor:
    lookup = dict(model.named_parameters())
    vparams = [lookup[n] for n in VIDEO_PARAMS]
    slot = VideoGradSlot([p.shape for p in vparams]) if all(p.requires_grad for p in vparams) else None
    out = _UpsampleVideoFunction.apply(model._dims, slot, video, *vparams)
    if slot is not None and out.requires_grad:
        out._mvn_video_slot = slot  # read back by wavenet_forward / wavenet_forward_loss
    return out


# ---- local conditioning on log-mel frames (csrc/features.hip) -------------------------------------------
def mel_filterbank(n_mels: int, n_fft: int, rate: float, f_min: float = 0.0, f_max: Optional[float] = None):
    """The (n_mels, n_fft // 2 + 1) float64 numpy filterbank mvn_logmel_frontend takes: HTK mel scale
    ``2595 log10(1 + f / 700)``, triangles between ``n_mels + 2`` equally spaced mel points from ``f_min`` to ``f_max``
    (default ``rate / 2``), evaluated at the bin frequencies ``k rate / n_fft``, peak 1, no area normalisation."""
    import numpy as np
    f_max = rate / 2.0 if f_max is None else float(f_max)
    if n_mels < 1 or n_fft < 2 or not 0.0 <= f_min < f_max <= rate / 2.0 + 1e-9:
        raise ValueError(f"mel_filterbank: need n_mels >= 1 and 0 <= f_min < f_max <= rate / 2, got n_mels={n_mels}, "
                         f"f_min={f_min}, f_max={f_max}, rate={rate}")

    def mel(f):
        return 2595.0 * np.log10(1.0 + np.asarray(f, dtype=np.float64) / 700.0)
    points = 700.0 * (10.0 ** (np.linspace(mel(f_min), mel(f_max), n_mels + 2) / 2595.0) - 1.0)
    freqs = np.arange(n_fft // 2 + 1, dtype=np.float64) * (float(rate) / n_fft)
    lo, mid, hi = points[:-2, None], points[1:-1, None], points[2:, None]
    return np.maximum(0.0, np.minimum((freqs[None, :] - lo) / (mid - lo), (hi - freqs[None, :]) / (hi - mid)))


def logmel_frames(n_samples: int, hop: int) -> int:
    """The frame count of ``logmel`` for a row of ``n_samples``: frames sit at 0, hop, 2 hop, ... <= n_samples."""
    return int(n_samples) // int(hop) + 1


_LOGMEL_TABLES: dict = {}


def _logmel_tables(device, n_fft: int):
    """(window, twiddle) of mvn_logmel_frontend on ``device``, made in float64 on the host once per (device, n_fft)."""
    key = (str(device), int(n_fft))
    if key not in _LOGMEL_TABLES:
        import numpy as np
        ang = 2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft
        window = 0.5 - 0.5 * np.cos(ang)
        twiddle = np.concatenate([np.cos(ang), np.sin(ang)])
        _LOGMEL_TABLES[key] = tuple(torch.from_numpy(t.astype(np.float32)).to(device) for t in (window, twiddle))
    return _LOGMEL_TABLES[key]


def logmel(indices: torch.Tensor, classes: int, n_fft: int, hop: int, fbank, floor: float = 1e-5,
           energies: bool = False) -> torch.Tensor:
    """(B, T) class indices on the GPU -> (B, n_mels, T // hop + 1) float32 log-mel frames of the waveform
    ``mu_law_decode`` gives (mvn_logmel_frontend: centred frames of ``n_fft`` samples, zeros outside the clip, periodic
    Hann window, power spectrum, ``fbank`` -- a (n_mels, n_fft // 2 + 1) array or tensor, e.g. ``mel_filterbank`` --
    floor, natural log).  ``energies``: the mel energies before floor and log.  Nothing here is differentiable."""
    _require_gpu(indices, "indices")
    if indices.dim() != 2 or indices.is_floating_point():
        raise ValueError(f"indices must be (batch, samples) integer classes, got {tuple(indices.shape)} {indices.dtype}")
    dev = indices.device
    idx = indices.detach().to(torch.int32).contiguous()
    fb = torch.as_tensor(fbank).detach().to(device=dev, dtype=torch.float32).contiguous()
    if fb.dim() != 2 or fb.shape[1] != int(n_fft) // 2 + 1:
        raise ValueError(f"fbank must be (n_mels, {int(n_fft) // 2 + 1}), got {tuple(fb.shape)}")
    B, T = idx.shape
    M, F = int(fb.shape[0]), logmel_frames(T, hop) if int(hop) >= 1 else 0
    lib = N.lib()
    with torch.cuda.device(dev):
        window, twiddle = _logmel_tables(dev, int(n_fft))
        out = torch.empty((B, M, max(F, 0)), dtype=torch.float32, device=dev)
        n = int(lib.mvn_logmel_scratch_floats(B, T, int(n_fft), int(hop)))
        scratch = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
        N.check(lib.mvn_logmel_frontend(idx.data_ptr(), B, T, int(classes), int(n_fft), int(hop), M, window.data_ptr(),
                                        twiddle.data_ptr(), fb.data_ptr(), float(floor), int(bool(energies)),
                                        out.data_ptr(), max(F, 1), scratch.data_ptr(), n, _stream_ptr(dev)),
                "mvn_logmel_frontend")
    return out


# ---- distance between two feature tensors (csrc/metrics.hip) --------------------------------------------
def distance_frame_span(lengths, T: int, n_fft: int, hop: int, skip: int = 0, batch: int = 1):
    """The frames of ``logmel`` that count in a spectral distance, as ``(first, count)``, two host lists of one int per
    sequence.  Frame f covers samples ``[f hop - h, f hop - h + n_fft)`` with ``h = n_fft // 2``; it counts when that
    window lies wholly inside ``[skip, len_b)``:

        first_b = ceil((skip + h) / hop),  last_b = floor((len_b - n_fft + h) / hop),
        count_b = max(0, min(last_b, F - 1) - first_b + 1),  F = logmel_frames(T, hop)

    ``skip`` keeps a copy-synthesis clip's prompt -- the source's own first samples -- from counting as a perfect
    match.  ``lengths``: as in ``valid_columns`` (its ValueErrors too), or None: each of ``batch`` rows is ``T``
    long.  Host integers only; nothing is launched."""
    T, n_fft, hop = int(T), int(n_fft), int(hop)
    if isinstance(skip, bool) or not isinstance(skip, int) or skip < 0:
        raise ValueError(f"skip must be an integer >= 0, got {skip!r}")
    if T < 1 or n_fft < 1 or hop < 1:
        raise ValueError(f"distance_frame_span: need T, n_fft and hop of at least 1, got {T}, {n_fft}, {hop}")
    values = [T] * int(batch) if lengths is None else _checked_lengths(lengths, T)
    h, F = n_fft // 2, logmel_frames(T, hop)
    first_f = -((-(skip + h)) // hop)  # ceil

    def count(n):
        last = (n - n_fft + h) // hop  # floor, also of a negative numerator
        return max(0, min(last, F - 1) - first_f + 1)
    return [first_f] * len(values), [count(v) for v in values]


def _span_values(values, name: str, B: int):
    """``first`` / ``count`` of ``feature_distance`` as a host list of B ints."""
    if isinstance(values, torch.Tensor):
        if values.dim() != 1 or values.is_floating_point() or values.is_complex() or values.dtype == torch.bool:
            raise ValueError(f"{name} must be a (batch,) integer tensor, got {tuple(values.shape)} {values.dtype}")
        values = values.detach().cpu().tolist()
    else:
        if isinstance(values, (str, bytes)) or not hasattr(values, "__len__") or getattr(values, "ndim", 1) != 1:
            raise ValueError(f"{name} must be a one-dimensional sequence of one integer per sequence, got {values!r}")
        values = values.tolist() if hasattr(values, "tolist") else list(values)
    if len(values) != B:
        raise ValueError(f"{name} names {len(values)} sequences, the batch holds {B}")
    for b, v in enumerate(values):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{name}[{b}] = {v!r} is not an integer")
    return values


def feature_distance(a: torch.Tensor, b: torch.Tensor, first=None, count=None, per_frame: bool = False) -> dict:
    """Log-spectral distance and mean absolute difference of two (B, M, F) float32 feature tensors on the GPU, e.g.
    two ``logmel`` outputs, over ONE span of frames per sequence (mvn_feature_distance; read only).  With
    ``d = a - b`` in double over frames ``[first_b, first_b + count_b)``:

        rms_f = sqrt(mean_m d^2),  lsd_db[b] = (10 / ln 10) mean_f rms_f,  l1[b] = mean_{f,m} |d|

    ``first`` / ``count``: host sequences, numpy arrays or integer tensors of B values (default: every frame).  Returns
    ``{"lsd_db": (B,) float64, "l1": (B,) float64, "frames": (B,) int32}`` and, on request, ``"per_frame"``: (B, F)
    float32, ``rms_f 10 / ln 10`` inside the span and exactly 0 outside it.  An empty span gives 0.0, never NaN.  No
    frame outside a span is read.  Every sum is formed in double in a fixed order: the same bits on every call, and
    a row's result does not depend on the other rows.  ValueError before any launch for a shape or dtype mismatch or
    a span that leaves [0, F]; RuntimeError for a CPU tensor."""
    _require_gpu(a, "a")
    _require_gpu(b, "b")
    if a.dim() != 3 or a.dtype != torch.float32 or min(a.shape) < 1:
        raise ValueError(f"a must be a (batch, bins, frames) float32 tensor with no empty axis, got {tuple(a.shape)} "
                         f"{a.dtype}")
    if tuple(b.shape) != tuple(a.shape) or b.dtype != torch.float32 or b.device != a.device:
        raise ValueError(f"b must be a {tuple(a.shape)} float32 tensor on {a.device}, got {tuple(b.shape)} {b.dtype} "
                         f"on {b.device}")
    B, M, F = (int(v) for v in a.shape)
    first = [0] * B if first is None else _span_values(first, "first", B)
    count = [F - f for f in first] if count is None else _span_values(count, "count", B)
    for s, (f0, n) in enumerate(zip(first, count)):
        if f0 < 0 or n < 0 or f0 + n > F:
            raise ValueError(f"the span of sequence {s}, first = {f0} and count = {n}, leaves the {F} frames")
    dev = a.device
    x, y = a.detach().contiguous(), b.detach().contiguous()
    lib = N.lib()
    with torch.cuda.device(dev):
        span = counts_to_device(first + count, dev)  # (one copy: first in front, count behind)
        out = {"lsd_db": torch.empty(B, dtype=torch.float64, device=dev),
               "l1": torch.empty(B, dtype=torch.float64, device=dev), "frames": span[B:]}
        if per_frame:
            out["per_frame"] = torch.empty(B, F, dtype=torch.float32, device=dev)
        n = int(lib.mvn_feature_distance_scratch_floats(B, F))
        scratch = torch.empty(max(n, 1) // 2 + 1, dtype=torch.float64, device=dev)  # (doubles: 8-byte aligned)
        N.check(lib.mvn_feature_distance(x.data_ptr(), y.data_ptr(), B, M, F, span.data_ptr(), span[B:].data_ptr(),
                                         out["lsd_db"].data_ptr(), out["l1"].data_ptr(),
                                         out["per_frame"].data_ptr() if per_frame else None, scratch.data_ptr(), n,
                                         _stream_ptr(dev)), "mvn_feature_distance")
    return out


# ---- pitch tracks and their distance (csrc/pitch.hip) ---------------------------------------------------
PITCH_MIN_WIN, PITCH_MAX_WIN, PITCH_MIN_LAG, PITCH_MAX_LAG, PITCH_MAX_HOP = 16, 4096, 2, 1024, 1 << 24


def pitch_lags(rate: float, f_min: float, f_max: float):
    """``(tau_min, tau_max) = (floor(rate / f_max), ceil(rate / f_min))``: the lags, in samples at ``rate``, of the
    periods of ``f_max`` .. ``f_min`` Hz.  A host function; ValueError unless 0 < f_min < f_max and rate > 0."""
    import math
    rate, f_min, f_max = float(rate), float(f_min), float(f_max)
    if not (rate > 0.0 and 0.0 < f_min < f_max) or math.isinf(rate) or math.isinf(f_max):
        raise ValueError(f"pitch_lags: need rate > 0 and 0 < f_min < f_max, got rate={rate}, f_min={f_min}, f_max={f_max}")
    return int(math.floor(rate / f_max)), int(math.ceil(rate / f_min))


def _whole(value, name: str) -> int:
    if isinstance(value, bool) or not isinstance(value, int):
        raise ValueError(f"{name} must be an integer, got {value!r}")
    return value


def check_pitch_settings(win, hop, tau_min, tau_max, threshold):
    """The settings of ``pitch`` as ``(win, hop, tau_min, tau_max, threshold)``; ValueError for what mvn_pitch_frames
    refuses of them."""
    win, hop, tau_min, tau_max = (_whole(v, n) for v, n in ((win, "win"), (hop, "hop"), (tau_min, "tau_min"),
                                                            (tau_max, "tau_max")))
    if not PITCH_MIN_WIN <= win <= PITCH_MAX_WIN:
        raise ValueError(f"win must lie in [{PITCH_MIN_WIN}, {PITCH_MAX_WIN}], got {win}")
    if not PITCH_MIN_LAG <= tau_max <= PITCH_MAX_LAG:
        raise ValueError(f"tau_max must lie in [{PITCH_MIN_LAG}, {PITCH_MAX_LAG}], got {tau_max}")
    if not 1 <= tau_min <= tau_max:
        raise ValueError(f"tau_min must lie in [1, tau_max = {tau_max}], got {tau_min}")
    if not 1 <= hop <= PITCH_MAX_HOP:
        raise ValueError(f"hop must lie in [1, 2^24], got {hop}")
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or not 0.0 < threshold <= 1.0:
        raise ValueError(f"threshold must lie in (0, 1], got {threshold!r}")
    return win, hop, tau_min, tau_max, float(threshold)


def pitch(indices_or_wave: torch.Tensor, classes: Optional[int] = None, *, win: int, hop: int, tau_min: int,
          tau_max: int, threshold: float = 0.15, cmnd: bool = False) -> dict:
    """The YIN pitch track of (B, T) audio on the GPU, one estimate per ``logmel`` frame (mvn_pitch_frames): an integer
    tensor is class indices, tracked on the waveform ``mu_law_decode(indices, classes)`` gives (an index outside
    [0, classes) is a 0.0 sample); a float32 tensor is the waveform itself and ``classes`` is not used.

    With L = win + tau_max, frame j covers samples [j hop - L // 2, j hop - L // 2 + L), zeros outside the row:
    ``distance_frame_span(lengths, T, L, hop, skip)`` names the frames that lie inside a clip.  Over that frame
    d(tau) = sum_{n < win} (x[n] - x[n + tau])^2, c(tau) = d(tau) tau / sum_{k <= tau} d(k) (1 where the sum is 0); the
    frame is voiced where some c(tau) < ``threshold`` for tau in [tau_min, tau_max] -- the pick is the first such dip's
    local minimum, refined by a parabola through its neighbours -- and unvoiced otherwise.

    Returns ``{"period": (B, F) float32 -- samples, exactly 0 where unvoiced --, "aper": (B, F) float32 -- c at the
    pick --}`` and with ``cmnd`` also ``"cmnd"``: (B, F, tau_max + 1) float32, c(0 .. tau_max) of every frame.  The same
    bits on every call and in every batch.  ValueError before any launch for a shape, dtype or range mvn_pitch_frames
    refuses; RuntimeError for a CPU tensor."""
    x = indices_or_wave
    _require_gpu(x, "indices_or_wave")
    if x.dim() != 2 or x.is_complex() or x.dtype == torch.bool or (x.is_floating_point() and x.dtype != torch.float32):
        raise ValueError(f"indices_or_wave must be (batch, samples) integer classes or a float32 waveform, got "
                         f"{tuple(x.shape)} {x.dtype}")
    win, hop, tau_min, tau_max, threshold = check_pitch_settings(win, hop, tau_min, tau_max, threshold)
    is_wave = x.is_floating_point()
    if not is_wave and (classes is None or _whole(classes, "classes") < 2):
        raise ValueError(f"class indices need classes >= 2, got {classes!r}")
    B, T = (int(v) for v in x.shape)
    if B > 65535 or T < 1 or T > 1 << 30 or B * T > 2 ** 31 - 1:
        raise ValueError(f"indices_or_wave {tuple(x.shape)}: need batch <= 65535, 1 <= samples <= 2^30 and at most "
                         "2^31 - 1 samples in all")
    dev = x.device
    x = x.detach().contiguous() if is_wave else x.detach().to(torch.int32).contiguous()
    F = logmel_frames(T, hop)
    lib = N.lib()
    with torch.cuda.device(dev):
        out = {"period": torch.empty((B, F), dtype=torch.float32, device=dev),
               "aper": torch.empty((B, F), dtype=torch.float32, device=dev)}
        if cmnd:
            out["cmnd"] = torch.empty((B, F, tau_max + 1), dtype=torch.float32, device=dev)
        n = int(lib.mvn_pitch_scratch_floats(B, T, win, tau_max))
        scratch = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
        N.check(lib.mvn_pitch_frames(None if is_wave else x.data_ptr(), x.data_ptr() if is_wave else None, B, T,
                                     0 if is_wave else int(classes), win, hop, tau_min, tau_max, threshold,
                                     out["period"].data_ptr(), out["aper"].data_ptr(),
                                     out["cmnd"].data_ptr() if cmnd else None, scratch.data_ptr(),
                                     n, _stream_ptr(dev)), "mvn_pitch_frames")
    return out


def pitch_distance(period_a: torch.Tensor, period_b: torch.Tensor, first=None, count=None,
                   gross_ratio: float = 0.2) -> dict:
    """F0 error of two (B, F) float32 period tracks on the GPU, e.g. two ``pitch`` outputs, over ONE span of frames per
    sequence (mvn_pitch_distance; read only).  A frame is voiced where its period is above 0.  Over the frames
    ``[first_b, first_b + count_b)``: ``voiced_frames`` are voiced in both tracks, ``vuv_errors`` in exactly one,
    ``f0_rmse_cents`` is the root mean square of ``1200 log2(period_b / period_a)`` over the former (0.0 where there
    are none), and ``gross_errors`` counts those with ``|period_a / period_b - 1| > gross_ratio``.

    ``first`` / ``count``: as in ``feature_distance`` (its span checks too; default: every frame).  Returns
    ``{"f0_rmse_cents": (B,) float64, "voiced_frames", "vuv_errors", "gross_errors", "frames": (B,) int32}``.  Sums in
    double in a fixed order; no frame outside a span is read.  ValueError before any launch for a shape or dtype
    mismatch, a span that leaves [0, F] or a ``gross_ratio`` that is not a finite number above 0; RuntimeError for a
    CPU tensor."""
    _require_gpu(period_a, "period_a")
    _require_gpu(period_b, "period_b")
    a, b = period_a, period_b
    if a.dim() != 2 or a.dtype != torch.float32 or min(a.shape) < 1:
        raise ValueError(f"period_a must be a (batch, frames) float32 tensor with no empty axis, got {tuple(a.shape)} "
                         f"{a.dtype}")
    if tuple(b.shape) != tuple(a.shape) or b.dtype != torch.float32 or b.device != a.device:
        raise ValueError(f"period_b must be a {tuple(a.shape)} float32 tensor on {a.device}, got {tuple(b.shape)} "
                         f"{b.dtype} on {b.device}")
    if isinstance(gross_ratio, bool) or not isinstance(gross_ratio, (int, float)) or not 0.0 < gross_ratio < float("inf"):
        raise ValueError(f"gross_ratio must be a finite number above 0, got {gross_ratio!r}")
    B, F = (int(v) for v in a.shape)
    if B > 65535:
        raise ValueError(f"at most 65535 sequences, got {B}")
    first = [0] * B if first is None else _span_values(first, "first", B)
    count = [F - f for f in first] if count is None else _span_values(count, "count", B)
    for s, (f0, n) in enumerate(zip(first, count)):
        if f0 < 0 or n < 0 or f0 + n > F:
            raise ValueError(f"the span of sequence {s}, first = {f0} and count = {n}, leaves the {F} frames")
    dev = a.device
    x, y = a.detach().contiguous(), b.detach().contiguous()
    with torch.cuda.device(dev):
        span = counts_to_device(first + count, dev)  # (one copy: first in front, count behind)
        rmse = torch.empty(B, dtype=torch.float64, device=dev)
        counts = torch.empty((B, 4), dtype=torch.int32, device=dev)
        N.check(N.lib().mvn_pitch_distance(x.data_ptr(), y.data_ptr(), B, F, span.data_ptr(), span[B:].data_ptr(),
                                           float(gross_ratio), rmse.data_ptr(), counts.data_ptr(), _stream_ptr(dev)),
                "mvn_pitch_distance")
    return {"f0_rmse_cents": rmse, "voiced_frames": counts[:, 0], "vuv_errors": counts[:, 1],
            "gross_errors": counts[:, 2], "frames": counts[:, 3]}


def pitch_of_classes(indices: torch.Tensor, classes: int, preemphasis: float = 0.0, **settings) -> dict:
    """``pitch`` of (B, T) class indices as the model's users hear them: at ``preemphasis`` A > 0 the tracker runs on
    the DE-EMPHASISED audio (``deemphasis_pcm16`` of the classes, over 32768, as a float32 waveform) -- pre-emphasis
    attenuates the fundamental, which is what a pitch tracker needs --, at A = 0 on the class indices as they are."""
    if preemphasis > 0.0:
        return pitch(deemphasis_pcm16(indices, preemphasis, classes).float() / 32768, **settings)
    return pitch(indices, classes, **settings)


# ---- a pitch track as local-conditioning channels (csrc/pitch_features.hip) ------------------------------
PITCH_FEATURES_CHUNK = 256  # the frames a workgroup of mvn_pitch_features scans at a time (kPfThreads)


def f0_reference(f_min: float, f_max: float) -> float:
    """``sqrt(f_min f_max)``: the frequency the log-F0 channel is 0 at, the middle of the search range in octaves.
    ValueError unless 0 < f_min < f_max, both finite."""
    import math
    f_min, f_max = float(f_min), float(f_max)
    if not 0.0 < f_min < f_max < math.inf:
        raise ValueError(f"f0_min and f0_max must be finite with 0 < f0_min < f0_max, got {f_min} and {f_max}")
    return math.sqrt(f_min * f_max)


def _shift_values(shift, B: int):
    """``shift`` of ``pitch_features`` as None (no shift) or a host list of B floats (octaves)."""
    if shift is None:
        return None
    if N.any_per_sequence(shift):
        values = shift.detach().cpu().tolist() if isinstance(shift, torch.Tensor) else \
            shift.tolist() if hasattr(shift, "tolist") else list(shift)
        if not isinstance(values, list) or any(isinstance(v, (list, tuple)) for v in values) or len(values) != B:
            raise ValueError(f"shift must be a number or one number per sequence ({B}), got {shift!r}")
    else:
        values = [shift.item() if isinstance(shift, torch.Tensor) else shift] * B
    for b, v in enumerate(values):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or v in (float("inf"), float("-inf")):
            raise ValueError(f"shift of sequence {b} is {v!r}, not a finite number")
    return None if all(v == 0 for v in values) else [float(v) for v in values]


def pitch_features(period: torch.Tensor, rate: float, f_ref: float, shift=None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A (B, F) float32 period track on the GPU, e.g. ``pitch(...)["period"]`` -- voiced where above 0 -- as two
    frame-rate conditioning channels (mvn_pitch_features):

        [:, -2]  the continuous log-F0 ``log2(rate / (period f_ref))`` (formed in double, rounded once), interpolated
                 linearly between the nearest voiced frames across an unvoiced gap, held at the first / last voiced
                 value in front of / behind them, 0 in a row without a voiced frame; plus ``shift`` octaves
        [:, -1]  1.0 where the frame is voiced, else 0.0

    ``shift``: None, a number, or one number per sequence (list, array or tensor).  ``out``: a float32 tensor
    (B, >= 2, >= F) with contiguous frames whose LAST TWO channels' first F frames are written -- nothing else of it is
    --, e.g. the (B, M + 2, F) features with the log-mel frames in front; default: a new (B, 2, F).  Returns ``out``.
    The same bits on every call and at every batch position.  ValueError before any launch for a shape, dtype or value
    mvn_pitch_features refuses; RuntimeError for a CPU tensor."""
    import math
    _require_gpu(period, "period")
    if period.dim() != 2 or period.dtype != torch.float32:
        raise ValueError(f"period must be a (batch, frames) float32 tensor, got {tuple(period.shape)} {period.dtype}")
    B, F = (int(v) for v in period.shape)
    if B > 65535 or F < 1 or F > 1 << 30:
        raise ValueError(f"period {tuple(period.shape)}: need batch <= 65535 and 1 <= frames <= 2^30")
    for name, v in (("rate", rate), ("f_ref", f_ref)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 < v < math.inf or \
                not 0.0 < ctypes.c_float(v).value < math.inf:
            raise ValueError(f"{name} must be a finite number above 0, got {v!r}")
    values = _shift_values(shift, B)
    dev = period.device
    if out is not None:
        _require_gpu(out, "out")
        if out.dim() != 3 or out.dtype != torch.float32 or out.device != dev or out.shape[0] != B or \
                out.shape[1] < 2 or out.shape[2] < F or (out.shape[2] > 1 and out.stride(2) != 1) or \
                out.stride(1) < F or (B > 1 and out.stride(0) < out.stride(1) + F):
            raise ValueError(f"out must be a ({B}, >= 2, >= {F}) float32 tensor on {dev} with contiguous frames and "
                             f"rows that do not overlap, got {tuple(out.shape)} {out.dtype} strides {out.stride()}")
    per = period.detach().contiguous()
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty((B, 2, F), dtype=torch.float32, device=dev)
        sh = None if values is None else torch.tensor(values, dtype=torch.float32).to(dev)
        rows = out[:, out.shape[1] - 2:]
        N.check(N.lib().mvn_pitch_features(per.data_ptr(), B, F, float(rate), float(f_ref),
                                           None if sh is None else sh.data_ptr(), rows.data_ptr(),
                                           out.stride(0) if B > 1 else out.stride(1) + F, out.stride(1),
                                           _stream_ptr(dev)), "mvn_pitch_features")
    return out


_MEL_FBANKS: dict = {}


def _record_fbank(device, record: dict) -> torch.Tensor:
    """The float32 ``mel_filterbank`` of a ``"local_conditioning"`` record on ``device``, made once per settings."""
    key = (str(device), int(record["local_channels"]), int(record["mel_fft"]), int(record["audio_rate"]),
           float(record["mel_fmin"]), float(record["mel_fmax"]))
    if key not in _MEL_FBANKS:
        fbank = mel_filterbank(key[1], key[2], key[3], key[4], key[5])
        _MEL_FBANKS[key] = torch.from_numpy(fbank).to(torch.float32).to(device)
    return _MEL_FBANKS[key]


@torch.no_grad()
def local_features(indices: torch.Tensor, classes: int, record: dict, shift=None, lengths=None,
                   preemphasis: float = 0.0) -> torch.Tensor:
    """(B, T) class indices on the GPU -> the local features of a model trained under ``record``, a checkpoint's
    ``"local_conditioning"`` record: the one place that turns audio into what ``forward`` / ``generate`` take as
    ``local_features``, for the trainer, its sample logger, ``synthesize`` and ``evaluate`` alike.

    Without an ``"f0"`` entry: ``logmel`` by the record's mel settings, (B, M, F) -- the same call, the same bits.
    With one (``--mel_f0 1``): (B, M + 2, F) -- channels 0 .. M - 1 are those log-mel frames, bit for bit (one device
    copy: mvn_logmel_frontend writes a tensor of its own width), and the last two are ``pitch_features`` of the YIN
    track taken at ``win = mel_fft``, ``hop = local_hop`` and ``pitch_lags(audio_rate, f_min, f_max)``, so a pitch
    frame is a log-mel frame.  ``preemphasis``: the model's (``pitch_of_classes``: the tracker hears the de-emphasised
    audio).  ``shift``: octaves added to the log-F0 channel, a number or one per sequence; a non-zero shift on a record
    without ``"f0"`` is a ValueError.  ``lengths`` (real samples per row, as in ``valid_columns``): a frame centred at
    or past its row's end counts as unvoiced whatever the tracker finds in the padding; the log-mel channels do not
    depend on it."""
    from .checkpoint import f0_record_of
    f0 = f0_record_of(record)
    mel = logmel(indices, classes, int(record["mel_fft"]), int(record["local_hop"]),
                 _record_fbank(indices.device, record))
    B, M, F = (int(v) for v in mel.shape)
    if f0 is None:
        if _shift_values(shift, B) is not None:
            raise ValueError("a pitch shift needs a checkpoint trained with --mel_f0 1: this local_conditioning record "
                             "has no 'f0' entry, the model has no F0 channel to shift")
        return mel
    rate, hop = int(record["audio_rate"]), int(record["local_hop"])
    tau_min, tau_max = pitch_lags(rate, float(f0["f_min"]), float(f0["f_max"]))
    period = pitch_of_classes(indices.detach().to(torch.int32).contiguous(), int(classes), float(preemphasis),
                              win=int(record["mel_fft"]), hop=hop, tau_min=tau_min, tau_max=tau_max)["period"]
    if lengths is not None:
        ends = counts_to_device([-(-v // hop) for v in _checked_lengths(lengths, int(indices.shape[1]))], mel.device)
        if int(ends.shape[0]) != B:
            raise ValueError(f"lengths names {int(ends.shape[0])} sequences, the batch holds {B}")
        period = period.masked_fill(torch.arange(F, device=mel.device)[None, :] >= ends[:, None], 0.0)
    with torch.cuda.device(mel.device):
        feats = torch.empty((B, M + 2, F), dtype=torch.float32, device=mel.device)
        feats[:, :M].copy_(mel)
    return pitch_features(period, float(rate), float(f0["f_ref"]), shift, out=feats)


class _UpsampleFeaturesFunction(torch.autograd.Function):
    """feats (B, M, F), W (C, M, taps) -- the conv's own weight -- and bias (C) -> context (B, C, T): taps = 1 through
    mvn_upsample_features, as ever; taps = 2 k + 1 > 1 through mvn_upsample_features_win."""

    @staticmethod
    def forward(ctx_, hop, T, feats, w, bias):
        lib = N.lib()
        dev = feats.device
        taps = int(w.shape[2])
        mel = feats.detach().to(torch.float32).contiguous()
        wf = (w[:, :, 0] if taps == 1 else w).detach().to(torch.float32).contiguous()
        bf = bias.detach().to(torch.float32).contiguous()
        B, M, F = mel.shape
        C = wf.shape[0]
        with torch.cuda.device(dev):
            ld = (T + 3) // 4 * 4  # rows start on 16 bytes
            buf = torch.empty((B, C, ld), dtype=torch.float32, device=dev)
            n = int(lib.mvn_upsample_features_scratch_floats(B, C, F))
            scratch = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
            if taps == 1:
                N.check(lib.mvn_upsample_features(mel.data_ptr(), mel.stride(1), wf.data_ptr(), bf.data_ptr(), B, M, F,
                                                  C, hop, T, buf.data_ptr(), ld, scratch.data_ptr(), n,
                                                  _stream_ptr(dev)), "mvn_upsample_features")
            else:
                N.check(lib.mvn_upsample_features_win(mel.data_ptr(), mel.stride(1), wf.data_ptr(), bf.data_ptr(), B, M,
                                                      F, C, taps, hop, T, buf.data_ptr(), ld, scratch.data_ptr(), n,
                                                      _stream_ptr(dev)), "mvn_upsample_features_win")
        ctx_.geom = (hop, T, taps)
        ctx_.save_for_backward(mel, wf)
        return buf[:, :, :T]

    @staticmethod
    def backward(ctx_, dout):
        lib = N.lib()
        mel, wf = ctx_.saved_tensors
        hop, T, taps = ctx_.geom
        B, M, F = mel.shape
        C = wf.shape[0]
        dev = mel.device
        dout = dout.to(torch.float32).contiguous()
        need_mel = ctx_.needs_input_grad[2]
        with torch.cuda.device(dev):
            dw = torch.zeros_like(wf)
            db = torch.zeros(C, dtype=torch.float32, device=dev)
            dmel = torch.empty_like(mel) if need_mel else None
            n = int(lib.mvn_upsample_features_scratch_floats(B, C, F))
            scratch = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
            if taps == 1:
                N.check(lib.mvn_upsample_features_backward(
                    dout.data_ptr(), dout.stride(1), mel.data_ptr(), mel.stride(1), wf.data_ptr(), B, M, F, C, hop, T,
                    dw.data_ptr(), db.data_ptr(), dmel.data_ptr() if need_mel else None, F, scratch.data_ptr(), n,
                    _stream_ptr(dev)), "mvn_upsample_features_backward")
                dw = dw[:, :, None]  # (the conv's (C, M, 1))
            else:
                N.check(lib.mvn_upsample_features_win_backward(
                    dout.data_ptr(), dout.stride(1), mel.data_ptr(), mel.stride(1), wf.data_ptr(), B, M, F, C, taps, hop,
                    T, dw.data_ptr(), db.data_ptr(), dmel.data_ptr() if need_mel else None, F, scratch.data_ptr(), n,
                    _stream_ptr(dev)), "mvn_upsample_features_win_backward")
        need = ctx_.needs_input_grad
        return None, None, dmel, dw if need[3] else None, db if need[4] else None


def local_frames_needed(T: int, hop: int) -> int:
    return (int(T) - 1) // int(hop) + 1


def check_local_features(model, local_features, batch: int, T: int) -> None:
    """The ValueErrors of ``local_features`` for a (batch, T) pass, before anything is launched: given to a model
    without ``local_channels``, missing on one with, a wrong shape, or too few frames for T."""
    M, hop = int(getattr(model, "local_channels", 0)), int(getattr(model, "local_hop", 0))
    if M <= 0:
        if local_features is not None:
            raise ValueError("local_features given to a model built without local_channels")
        return
    if local_features is None:
        raise ValueError(f"this model was built with local_channels={M}: local_features is required")
    if not torch.is_tensor(local_features) or local_features.dim() != 3 or not local_features.is_floating_point():
        raise ValueError(f"local_features must be a ({batch}, {M}, frames) float tensor")
    if local_features.shape[0] != batch or local_features.shape[1] != M:
        raise ValueError(f"local_features must be ({batch}, {M}, frames), got {tuple(local_features.shape)}")
    need = local_frames_needed(T, hop)
    if local_features.shape[2] < need:
        raise ValueError(f"local_features holds {local_features.shape[2]} frames; {T} samples at hop {hop} need {need}")


def upsample_features(model, feats: torch.Tensor, T: int) -> torch.Tensor:
    """``feats`` (B, local_channels, F) -> the (B, C, T) context of ``model.local_conv`` applied at frame rate and
    interpolated linearly between frames ``model.local_hop`` samples apart (mvn_upsample_features); differentiable in
    ``feats`` and in the conv's weight and bias.  A conv of kernel size 2 k + 1 > 1 (``local_window = k``) sees k frames
    on each side of a frame, the edge frames repeated past the ends of ``feats`` (mvn_upsample_features_win)."""
    check_local_features(model, feats, int(feats.shape[0]) if torch.is_tensor(feats) and feats.dim() == 3 else -1, T)
    _require_gpu(feats, "local_features")
    if int(T) < 1:
        raise ValueError(f"upsample_features: T must be at least 1, got {T}")
    conv = model.local_conv
    return _UpsampleFeaturesFunction.apply(int(model.local_hop), int(T), feats, conv.weight, conv.bias)


@torch.no_grad()
def project_features(model, feats: torch.Tensor) -> torch.Tensor:
    """``feats`` (B, local_channels, F) -> (B, C, F) fp32: ``model.local_conv`` applied at frame rate, the edge frames
    repeated past the ends of ``feats`` (mvn_project_features) -- what ``upsample_features`` interpolates between,
    kept, to the bit.  Not differentiable: the source of a windowed generator context."""
    check_local_features(model, feats, int(feats.shape[0]) if torch.is_tensor(feats) and feats.dim() == 3 else -1, 1)
    _require_gpu(feats, "local_features")
    conv = model.local_conv
    mel = feats.detach().to(torch.float32).contiguous()
    w = conv.weight.detach().to(torch.float32).contiguous()  # (C, M, taps)
    b = conv.bias.detach().to(torch.float32).contiguous()
    B, M, F = mel.shape
    C, taps = int(w.shape[0]), int(w.shape[2])
    with torch.cuda.device(mel.device):
        proj = torch.empty((B, C, F), dtype=torch.float32, device=mel.device)
        N.check(N.lib().mvn_project_features(mel.data_ptr(), mel.stride(1), w.data_ptr(), b.data_ptr(), B, M, F, C,
                                             taps, proj.data_ptr(), F, _stream_ptr(mel.device)), "mvn_project_features")
    return proj


@torch.no_grad()
def context_window(proj, hop: int, t0: int, n: int, glob=None, proj_rows=None, out=None) -> torch.Tensor:
    """Columns [t0, t0 + n) of the generators' time-major context, (rows, n, C) fp32 (mvn_context_window): ``proj``
    (proj_rows, C, F) from ``project_features`` interpolated between frames ``hop`` samples apart, plus ``glob``
    (rows, C), the label's vectors; either may be None (not both) -- ``proj`` None is the label-only window.  Row r
    reads ``proj[r % proj_rows]`` (default: ``proj``'s rows), so the two rows of a guided pair share a projection;
    rows = ``glob``'s, else ``out``'s, else ``proj``'s.  ``out``: a contiguous fp32 tensor of at least rows * n * C
    elements to write into (its first rows * n * C are the result).  The bits are those of ``upsample_features`` ->
    ``mvn_transpose_context`` -> ``mvn_context_add_global``.  Not differentiable."""
    if proj is None and glob is None:
        raise ValueError("context_window: proj and glob are both None")
    src = proj if proj is not None else glob
    _require_gpu(src, "context_window's source")
    dev = src.device
    if proj is not None:
        if proj.dim() != 3 or proj.dtype != torch.float32:
            raise ValueError(f"proj must be (rows, C, frames) float32, got {tuple(proj.shape)} {proj.dtype}")
        if proj.stride(2) != 1 or proj.stride(0) != proj.shape[1] * proj.stride(1):
            proj = proj.contiguous()
    C = int(proj.shape[1]) if proj is not None else int(glob.shape[1])
    if glob is not None:
        if glob.dim() != 2 or int(glob.shape[1]) != C or glob.dtype != torch.float32 or glob.device != dev:
            raise ValueError(f"glob must be (rows, {C}) float32 on {dev}, got {tuple(glob.shape)} {glob.dtype}")
        glob = glob.contiguous()
    if proj_rows is None:
        proj_rows = int(proj.shape[0]) if proj is not None else 1
    if proj is not None and not 1 <= int(proj_rows) <= int(proj.shape[0]):
        raise ValueError(f"proj_rows must lie in [1, {int(proj.shape[0])}], got {proj_rows}")
    rows = int(glob.shape[0]) if glob is not None else int(out.shape[0]) if out is not None and out.dim() == 3 \
        else int(proj.shape[0])
    t0, n = int(t0), int(n)
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty((rows, max(n, 0), C), dtype=torch.float32, device=dev)
        elif out.dtype != torch.float32 or out.device != dev or not out.is_contiguous() or \
                out.numel() < rows * max(n, 0) * C:
            raise ValueError(f"out must be a contiguous float32 tensor of at least {rows * max(n, 0) * C} elements "
                             f"on {dev}")
        N.check(N.lib().mvn_context_window(
            None if proj is None else proj.data_ptr(), 1 if proj is None else proj.stride(1), int(proj_rows),
            1 if proj is None else int(proj.shape[2]), None if glob is None else glob.data_ptr(), rows, C, int(hop),
            t0, n, out.data_ptr(), _stream_ptr(dev)), "mvn_context_window")
    return out.view(-1)[:rows * n * C].view(rows, n, C)


_BIAS_WITH_VIDEO = "global_path 'bias' runs models without a video context"


def plan_sequence(model, has_video: bool, has_label: bool) -> SequenceMode:
    """Phase one of a pass's plan, shape-free: the precision ``model`` asks for and every ValueError that needs only
    the model's attributes and whether a video / a label is given -- raised before the video encoder runs (the bf16
    entry points refuse the same).  bf16 runs C = K = 64; a video context only where the model opts in a second time
    (``bf16_context = True``; labels then ride in the context); labels without video only on the one-vector-per-layer
    path, asked for by name (``global_path = "bias"``).  "bias" never runs with video."""
    precision = getattr(model, "forward_precision", "fp32")
    path = getattr(model, "global_path", "auto")
    if precision == "bf16":
        C, K = model._dims.residual_channels, model._dims.skip_channels
        if C != 64 or K != 64:
            raise ValueError("forward_precision 'bf16' needs residual_channels = skip_channels = 64, "
                             f"got {C} and {K}")
        if has_video and not getattr(model, "bf16_context", False):
            raise ValueError("forward_precision 'bf16' runs audio-only models: no video context")
        if has_label and not has_video and path != "bias":
            raise ValueError("forward_precision 'bf16' runs audio-only models: no global conditioning (global_features) "
                             "unless global_path is 'bias'")
    if has_label and has_video and path == "bias":
        raise ValueError(_BIAS_WITH_VIDEO)
    return SequenceMode(precision=precision)


def bf16_mode(model, conditioned: bool, labelled: bool = False) -> bool:
    """Whether ``model.forward_precision`` is 'bf16' -- then with plan_sequence's ValueErrors; else nothing is checked."""
    return (getattr(model, "forward_precision", "fp32") == "bf16"
            and plan_sequence(model, conditioned, labelled).precision == "bf16")


def global_vector(model, global_features, batch: int):
    """The (B, C) global vectors e_b of ``global_features``, or None for a model built without
    ``global_classes`` (the argument is then ignored, as the reference ignores it).  (B,) integers index the rows of
    ``global_embedding.weight``; a (B, G) float tensor mixes them (one-hot, or a blend of styles).  ValueError, before
    anything is launched, for a missing argument, a wrong length / width or an index outside [0, G)."""
    G = int(getattr(model, "global_classes", 0))
    if G <= 0:
        return None
    if global_features is None:
        raise ValueError(f"this model was built with global_classes={G}: global_features is required")
    E = model.global_embedding.weight
    gf = global_features if torch.is_tensor(global_features) else torch.as_tensor(global_features)
    if gf.dim() == 1 and not gf.is_floating_point() and gf.dtype != torch.bool:
        if gf.shape[0] != batch:
            raise ValueError(f"global_features has {gf.shape[0]} entries for a batch of {batch}")
        host = gf.detach().cpu()
        if batch and (int(host.min()) < 0 or int(host.max()) >= G):
            raise ValueError(f"global_features holds a class outside [0, {G}): {host.tolist()}")
        return E[gf.to(device=E.device, dtype=torch.int64)]
    if gf.dim() == 2 and gf.is_floating_point():
        if gf.shape[0] != batch or gf.shape[1] != G:
            raise ValueError(f"global_features must be ({batch},) class indices or ({batch}, {G}) rows, "
                             f"got {tuple(gf.shape)}")
        return gf.to(device=E.device, dtype=E.dtype) @ E
    raise ValueError(f"global_features must be ({batch},) integer class indices or ({batch}, {G}) float rows, "
                     f"got {tuple(gf.shape)} {gf.dtype}")


def place_sequence(model, mode: SequenceMode, context, gvec, batch: int, t_len: int, loss_rule=None):
    """Phase two, for a (batch, t_len): the finished mode and the (context, gvec) pair the autograd nodes take.
    A label takes the one-vector-per-layer path ("bias": the vectors go in as they are) where ``model.global_path ==
    "bias"`` requires it -- ValueError where it does not exist -- or where "auto" finds it: fp32, C = K = 64, no video,
    and the row's path query grants the shape under the process's kernel switches.  Anywhere else it joins the context
    as a column constant in time.  ``loss_rule``: the fused loss node's, which trains fp32 under precision 'fp16'."""
    dims, path = model._dims, getattr(model, "global_path", "auto")
    labelled, bias = gvec is not None, False
    c64 = dims.residual_channels == 64 and dims.skip_channels == 64
    if labelled and path == "bias":
        if context is not None:
            raise ValueError(_BIAS_WITH_VIDEO)
        if not c64:
            raise ValueError("global_path 'bias' needs residual_channels = skip_channels = 64, "
                             f"got {dims.residual_channels} and {dims.skip_channels}")
        if (mode.precision, "bias") not in SEQUENCE_ENTRIES:
            raise ValueError(f"global_path 'bias' runs forward_precision 'fp32' or 'bf16', not {mode.precision!r}")
    if labelled and (path == "bias" or (path == "auto" and context is None and mode.precision == "fp32" and c64)):
        ask = SEQUENCE_ENTRIES[mode.precision, "bias"].path_query
        with torch.cuda.device(gvec.device):
            bias = getattr(N.lib(), ask)(dims, batch, t_len) == 1
        if path == "bias" and not bias:
            raise ValueError(f"global_path 'bias': the {mode.precision} layer kernels do not run batch {batch}, length "
                             f"{t_len} under the process's kernel switches ({ask} returned 0)")
    if labelled and not bias:
        slot = getattr(context, "_mvn_video_slot", None)
        context = gvec[:, :, None].expand(-1, -1, t_len) if context is None else context + gvec[:, :, None]
        if slot is not None:
            context._mvn_video_slot = slot
        gvec = None
    mode = mode._replace(
        precision="fp32" if loss_rule is not None and mode.precision == "fp16" else mode.precision,
        conditioning="bias" if bias else "none" if context is None else "context",
        label_in_context=labelled and not bias,
        loss_rule=N.LOSS_REFERENCE if loss_rule is None else loss_rule,
        grad_mode=torch.is_grad_enabled(),
        video_slot=None if context is None else getattr(context, "_mvn_video_slot", None))
    return mode, context, gvec


def _decoder_params(model, with_context: bool):
    L = model.layer_size * model.stack_size
    names = decoder_param_names(L, with_context=with_context)
    lookup = dict(model.named_parameters())
    return names, [lookup[n] for n in names]


def wavenet_forward(model, audio: torch.Tensor, context=None, output_unnormalized: bool = True,
                    remove_last: bool = True, gvec=None) -> torch.Tensor:
    """WaveNet.forward.  NOTE the reference's inverted flag (wavenet.py:189-191):
    output_unnormalized=True returns PROBABILITIES.  ``context``: upsampled video
    (B, C, T) or None.  One-hot input runs the causal conv as a gather; the check that the
    input IS one-hot is read after the kernels have been enqueued (no host wait on an idle
    GPU) and anything else is rerun through the dense causal conv."""
    mode = plan_sequence(model, context is not None, gvec is not None)
    model.compute_output_size(audio)  # ValueError when T < RF, like the reference
    mode, context, gvec = place_sequence(model, mode, context, gvec, int(audio.shape[0]), int(audio.shape[2]))
    idx, check = model._indices_async(audio)
    names, params = _decoder_params(model, mode.conditioning != "none")
    out = _WaveNetFunction.apply(mode, model._dims, names, idx, bool(output_unnormalized),
                                 bool(remove_last), context, gvec, *params)
    if not model._all_one_hot(check):  # dense causal conv on the tensor itself
        # (a dense input pays the discarded index pass: one extra forward; its buffers --
        # saved activations included -- are released BEFORE the rerun allocates its own)
        del out
        dense = audio.detach().to(torch.float32).contiguous()
        out = _WaveNetFunction.apply(mode, model._dims, names, dense, bool(output_unnormalized),
                                     bool(remove_last), context, gvec, *params)
    return out if audio.dtype == torch.float32 else out.to(audio.dtype)


def wavenet_forward_loss(model, audio: torch.Tensor, context=None, target=None, loss_rule=None, gvec=None,
                         lengths=None):
    """(loss, accuracy, probabilities) of one trainer step in one autograd node:
    ``output = model(audio, video)`` (probabilities, Q1), ``target =
    audio[:, :, RF:].argmax(1)``, ``F.cross_entropy(output, target)`` (on probabilities, Q2) and
    the accuracy -- movenet/pytorch_lightning_trainer.py:62-66 -- with the softmax, the loss and
    the accuracy fused into one pass over the head's logits and their gradients into one pass
    back.  Same values as ``cross_entropy_on_probs(wavenet_forward(...), target)``.

    ``loss_rule`` ("reference" / "model"; default: ``model.loss_rule``): under "model" the loss is
    ``F.cross_entropy(logits, target)`` instead -- the mean negative log-likelihood, in nats, of the
    distribution ``generate_sampling = "model"`` draws from; accuracy and probabilities are the same.

    ``lengths`` ((B,) host sequence or integer tensor; default None: every column counts, today's calls): sequence b
    holds ``lengths[b]`` real samples and padding behind them.  Loss and accuracy are then sums over the valid
    columns (``valid_columns``) divided by ``max(N_valid, 1)``, and d loss / d logits is exactly 0 on every other
    column (mvn_softmax_ce_*_len).  A host sequence adds no synchronisation: the divisor is formed on the host."""
    rule = N.loss_rule(getattr(model, "loss_rule", "reference") if loss_rule is None else loss_rule)
    mode = plan_sequence(model, context is not None, gvec is not None)
    model.compute_output_size(audio)
    valid = _valid_for_batch(lengths, int(audio.shape[0]), int(audio.shape[2]), model.receptive_fields)
    if valid is not None:
        _require_gpu(audio, "audio")
        valid = (counts_to_device(valid, audio.device), 1.0 / max(sum(valid), 1))
    mode, context, gvec = place_sequence(model, mode, context, gvec, int(audio.shape[0]), int(audio.shape[2]),
                                         loss_rule=rule)
    rf = model.receptive_fields
    idx, check = model._indices_async(audio)
    names, params = _decoder_params(model, mode.conditioning != "none")
    tg = idx[:, rf:].to(torch.int64) if target is None else target
    res = _WaveNetLossFunction.apply(mode, model._dims, names, idx, tg, valid, context, gvec, *params)
    if not model._all_one_hot(check):  # (read after the enqueue: no idle GPU) dense causal conv
        del res  # release the discarded pass (saved activations) before the rerun allocates
        dense = audio.detach().to(torch.float32).contiguous()
        tg = audio[:, :, rf:].argmax(1) if target is None else target
        res = _WaveNetLossFunction.apply(mode, model._dims, names, dense, tg, valid, context, gvec, *params)
    return res


def score_temperature(temperature) -> float:
    """``temperature`` of the scoring calls as a float; ValueError unless it is a finite number above 0."""
    if (isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not temperature > 0
            or temperature == float("inf")):
        raise ValueError(f"temperature must be a finite number above 0, got {temperature!r}")
    return float(temperature)


def score_logits(logits: torch.Tensor, target: torch.Tensor, temperature: float = 1.0, entropy: bool = False,
                 rank: bool = False, valid=None) -> dict:
    """Per-position log-likelihood of ``target`` under ``softmax(logits / temperature)`` in one read-only pass over
    the logits (mvn_score_columns): no probability tensor, ``logits`` untouched.  ``logits`` (B, Q, S) float32 on the
    GPU, ``target`` (B, S) integer classes (clamped to [0, Q-1]).  Returns a dict: ``logp`` (B, S) in nats,
    ``seq_nll`` (B,) = -logp.sum(1), ``seq_correct`` (B,) int32 = the columns whose target is the first maximum, and
    on request ``entropy`` (B, S) of the distribution and ``rank`` (B, S) int32 of the target in it (0: the first
    maximum).  The sums are formed in a fixed order: the same bits on every call.  ``valid`` ((B,) int32 on the
    logits' device; default None: every column counts): sequence b counts its first ``valid[b]`` columns only -- the
    others come back as logp = entropy = 0, rank = -1 and stay out of the sums (mvn_score_columns_len).  ValueError /
    RuntimeError before any launch for a bad temperature, a shape mismatch or a CPU tensor."""
    temperature = score_temperature(temperature)
    _require_gpu(logits, "logits")
    if logits.dim() != 3 or logits.dtype != torch.float32:
        raise ValueError(f"logits must be a (batch, classes, positions) float32 tensor, got {tuple(logits.shape)} "
                         f"{logits.dtype}")
    B, Q, S = logits.shape
    if tuple(target.shape) != (B, S) or target.is_floating_point() or target.dtype == torch.bool:
        raise ValueError(f"target must be ({B}, {S}) integer classes, got {tuple(target.shape)} {target.dtype}")
    _require_gpu(target, "target")
    if Q < 1:
        raise ValueError("logits hold no classes")
    dev = logits.device
    if valid is not None and (not isinstance(valid, torch.Tensor) or tuple(valid.shape) != (B,)
                              or valid.dtype != torch.int32 or valid.device != dev):
        raise ValueError(f"valid must be a ({B},) int32 tensor on {dev}")
    x = logits.detach().contiguous()
    tg = target.detach().to(device=dev, dtype=torch.int64).contiguous()
    lib = N.lib()
    with torch.cuda.device(dev):
        out = {"logp": torch.empty(B, S, dtype=torch.float32, device=dev),
               "seq_nll": torch.empty(B, dtype=torch.float32, device=dev),
               "seq_correct": torch.empty(B, dtype=torch.int32, device=dev)}
        if entropy:
            out["entropy"] = torch.empty(B, S, dtype=torch.float32, device=dev)
        if rank:
            out["rank"] = torch.empty(B, S, dtype=torch.int32, device=dev)
        n = lib.mvn_score_scratch_floats(B, S)
        scratch = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
        args = (x.data_ptr(), tg.data_ptr(), B, Q, S, temperature, out["logp"].data_ptr(),
                out["entropy"].data_ptr() if entropy else None, out["rank"].data_ptr() if rank else None,
                out["seq_nll"].data_ptr(), out["seq_correct"].data_ptr(), scratch.data_ptr(), n)
        if valid is None:
            N.check(lib.mvn_score_columns(*args, _stream_ptr(dev)), "mvn_score_columns")
        else:
            N.check(lib.mvn_score_columns_len(*args, valid.contiguous().data_ptr(), _stream_ptr(dev)),
                    "mvn_score_columns_len")
    return out


def wavenet_score(model, audio: torch.Tensor, context=None, gvec=None, temperature: float = 1.0,
                  entropy: bool = False, rank: bool = False, valid=None) -> dict:
    """``score_logits`` of the model's own logits for ``audio`` against ``audio[:, :, RF:]`` (WaveNet.score): the
    forward's checks and kernels -- whatever ``forward_precision`` and ``global_path`` say -- with nothing saved and
    nothing normalised, then mvn_score_columns on what the head wrote."""
    temperature = score_temperature(temperature)
    mode = plan_sequence(model, context is not None, gvec is not None)
    model.compute_output_size(audio)  # ValueError when T < RF
    idx, check = model._indices_async(audio)
    out = score_indices(model, idx, context, gvec, temperature, entropy, rank, mode, valid=valid)
    if not model._all_one_hot(check):  # (read after the enqueue, as forward reads it)
        raise ValueError("WaveNet.score expects one-hot audio (the target is its class index): a column of the input "
                         "is not one-hot")
    return out


def score_indices(model, idx: torch.Tensor, context, gvec, temperature: float, entropy: bool, rank: bool,
                  mode: SequenceMode, valid=None) -> dict:
    """The scoring pass on class indices ``idx`` (B, T) int32 (what WaveNet.score and WaveNet.classify share);
    ``mode``: plan_sequence's, placed here for the chunk's batch."""
    B, T = idx.shape
    mode, context, gvec = place_sequence(model, mode, context, gvec, B, T)
    names, params = _decoder_params(model, mode.conditioning != "none")
    sd = {n: p.detach() for n, p in zip(names, params)}
    if gvec is not None:
        gvec = gvec.detach().to(torch.float32).contiguous()
    logits, _ = run_forward(model._dims, sd, idx, False, True, False, mode, context if gvec is None else gvec)
    return score_logits(logits, idx[:, model.receptive_fields:], temperature, entropy=entropy, rank=rank,
                        valid=valid)


def mu_law_encode(x: torch.Tensor, quantization_channels: int) -> torch.Tensor:
    """float waveform in [-1, 1] (any shape, on the GPU) -> int32 class indices."""
    _require_gpu(x, "waveform")
    x = x.detach().to(torch.float32).contiguous()
    out = torch.empty(x.shape, dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        N.check(N.lib().mvn_mu_law_encode(x.data_ptr(), out.data_ptr(), x.numel(),
                                          quantization_channels, _stream_ptr(x.device)),
                "mvn_mu_law_encode")
    return out


def mu_law_decode(index: torch.Tensor, quantization_channels: int) -> torch.Tensor:
    _require_gpu(index, "indices")
    index = index.detach().to(torch.int32).contiguous()
    out = torch.empty(index.shape, dtype=torch.float32, device=index.device)
    with torch.cuda.device(index.device):
        N.check(N.lib().mvn_mu_law_decode(index.data_ptr(), out.data_ptr(), index.numel(),
                                          quantization_channels, _stream_ptr(index.device)),
                "mvn_mu_law_decode")
    return out


def pcm16_chunk(samples: torch.Tensor, t0: int, n: int, classes: int, out: Optional[torch.Tensor] = None,
                deemphasis: float = 0.0, state: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Columns [t0, t0 + n) of (batch, T) int32 class indices on the GPU -> (batch, n) int16 PCM on the GPU
    (mvn_pcm16_chunk): to the bit what ``callbacks.write_wav`` stores for ``mu_law_decode`` of those classes, a class
    outside [0, classes) clamped.  ``samples`` may be a row block or column view of a larger tensor (its last
    dimension contiguous); ``out``: an int16 tensor of at least (batch, n) whose first n columns are written.

    ``deemphasis`` = a in (0, 1) (mvn_pcm16_deemph_chunk; 0, the default, is the call above, untouched): the decoded
    samples go through y[t] = (1 + a) x[t] + a y[t-1] in float64 before the rounding -- the inverse of the front
    end's ``preemphasis`` -- with y[t-1] of each row carried in ``state``, a (batch,) float64 tensor on the GPU that the
    caller zeroes before a clip's column 0 and hands to every later chunk of that clip.  The PCM does not depend on how
    the clip is cut into chunks."""
    a = N.emphasis(deemphasis, "deemphasis")
    if a > 0.0:
        if state is None:
            raise ValueError("deemphasis > 0 needs state: a (batch,) float64 tensor on the GPU, zero before column 0")
        _require_gpu(state, "state")
    _require_gpu(samples, "samples")
    if samples.dim() != 2 or samples.dtype != torch.int32 or (samples.shape[1] > 1 and samples.stride(1) != 1):
        raise ValueError(f"samples must be (batch, T) int32 with contiguous rows, got {tuple(samples.shape)} "
                         f"{samples.dtype}")
    B, T = samples.shape
    t0, n = int(t0), int(n)
    if t0 < 0 or n < 0 or t0 + n > T:
        raise ValueError(f"columns [{t0}, {t0 + n}) do not lie inside the {T} of samples")
    if a > 0.0 and (tuple(state.shape) != (B,) or state.dtype != torch.float64 or not state.is_contiguous()
                    or state.device != samples.device):
        raise ValueError(f"state must be a contiguous ({B},) float64 tensor on {samples.device}")
    if out is None:
        out = torch.empty((B, n), dtype=torch.int16, device=samples.device)
    else:
        _require_gpu(out, "out")
        if out.dim() != 2 or out.dtype != torch.int16 or out.shape[0] != B or out.shape[1] < n or \
                (out.shape[1] > 1 and out.stride(1) != 1) or out.device != samples.device:
            raise ValueError(f"out must be ({B}, >= {n}) int16 with contiguous rows on {samples.device}")
    if B == 0 or n == 0:
        return out[:, :n]
    # (the row stride bounds what a launch may read of a row: a view's last row ends at its own T columns)
    stride = samples.stride(0) if B > 1 else T
    if stride < T or (B > 1 and out.stride(0) < n):
        raise ValueError("samples / out: rows overlap")
    pcm_stride = out.stride(0) if B > 1 else max(out.shape[1], n)
    with torch.cuda.device(samples.device):
        if a > 0.0:
            N.check(N.lib().mvn_pcm16_deemph_chunk(samples.data_ptr(), B, stride, t0, n, int(classes), a,
                                                   state.data_ptr(), out.data_ptr(), pcm_stride,
                                                   _stream_ptr(samples.device)), "mvn_pcm16_deemph_chunk")
        else:
            N.check(N.lib().mvn_pcm16_chunk(samples.data_ptr(), B, stride, t0, n, int(classes), out.data_ptr(),
                                            pcm_stride, _stream_ptr(samples.device)), "mvn_pcm16_chunk")
    return out[:, :n]


def deemphasis_pcm16(classes: torch.Tensor, a: float, quantization_channels: int) -> torch.Tensor:
    """Whole clips: (batch, T) int32 class indices on the GPU -> (batch, T) int16 PCM through the de-emphasis filter
    from a zero state (``pcm16_chunk`` with ``deemphasis=a`` over all columns) -- the bits a stream of the same classes
    delivers chunk by chunk.  ``a == 0`` is plain ``pcm16_chunk``."""
    _require_gpu(classes, "classes")
    state = torch.zeros(classes.shape[0], dtype=torch.float64, device=classes.device) if a > 0 else None
    return pcm16_chunk(classes, 0, classes.shape[1], quantization_channels, deemphasis=a, state=state)


AUDIO_FRONTEND_MAX_RATIO = 100  # frames <= 100 n_out: the longest clip whose output tile's window fits the LDS


_AUDIO_CLIP = [("offset", "<i8"), ("frames", "<i4"), ("channels", "<i4")]
_AUDIO_CLIP_VAR = _AUDIO_CLIP + [("n_out", "<i4"), ("reserved", "<i4")]
_AUDIO_CLIP_WINDOW = [("offset", "<i8"), ("span_first", "<i8"), ("out_first", "<i8"), ("file_frames", "<i8"),
                      ("span_frames", "<i4"), ("channels", "<i4"), ("n_out", "<i4"), ("rate_in", "<i4"),
                      ("rate_out", "<i4"), ("lo", "<f4"), ("hi", "<f4"), ("reserved", "<i4")]


def _back_to_back(spans, offsets=None):
    """A descriptor array's ``offsets`` as given, else those of ``spans`` (int64 elements each) lying back to back in
    the upload"""
    import numpy as np
    if offsets is not None:
        return offsets
    return np.concatenate([[0], np.cumsum(spans)[:-1]]) if len(spans) else []


def audio_clip_descriptors(frames, channels, offsets=None):
    """Host array of mvn_audio_clip records (int64 offset, int32 frames, int32 channels) as (B, 4) int32;
    ``offsets`` default to the clips lying back to back in the upload."""
    import numpy as np
    rec = np.zeros(len(frames), dtype=_AUDIO_CLIP)
    rec["frames"], rec["channels"] = frames, channels
    rec["offset"] = _back_to_back(rec["frames"].astype(np.int64) * rec["channels"], offsets)
    return rec.view(np.int32).reshape(len(frames), 4)


def _check_pcm(pcm: torch.Tensor) -> None:
    _require_gpu(pcm, "pcm")
    if pcm.dtype != torch.int16 or pcm.dim() != 1 or not pcm.is_contiguous():
        raise ValueError("pcm must be a contiguous 1-D int16 tensor")


_AUDIO_FORMS = {"mvn_audio_frontend": N.AUDIO_FORM_CLIP, "mvn_audio_frontend_var": N.AUDIO_FORM_VAR,
                "mvn_audio_frontend_window": N.AUDIO_FORM_WINDOW}


def _audio_frontend_call(entry: str, scratch_entry: str, pcm, descriptors, words: int, B, Q, width, normalize,
                         y=None, idx=None, preemphasis: float = 0.0):
    """One launch pair of the front end through ``entry`` (all three share one kernel pair, see csrc/audio.hip):
    ``descriptors`` a (B, words) int32 tensor on the GPU, B its own row count where None; ``y`` / ``idx`` the
    (B, width) outputs where the caller brings them.  Returns (idx, y, None) -- with ``preemphasis`` > 0, through
    mvn_audio_frontend_emph in ``entry``'s form, (idx, y, e): the indices of the pre-emphasised rows and those rows."""
    a = N.emphasis(preemphasis)
    _check_pcm(pcm)
    _require_gpu(descriptors, "descriptors")
    if B is None and descriptors.dim() == 2:
        B = int(descriptors.shape[0])
    if B is None or B < 1 or tuple(descriptors.shape) != (B, words) or descriptors.dtype != torch.int32 \
            or not descriptors.is_contiguous():
        raise ValueError(f"descriptors must be a contiguous (B, {words}) int32 tensor")
    dev, lib = pcm.device, N.lib()
    with torch.cuda.device(dev):
        y = torch.empty(B, width, dtype=torch.float32, device=dev) if y is None else y
        idx = torch.empty(B, width, dtype=torch.int32, device=dev) if idx is None else idx
        for t, dt, what in ((y, torch.float32, "waveform_out"), (idx, torch.int32, "out")):
            if tuple(t.shape) != (B, width) or t.dtype != dt or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"{what} must be a contiguous ({B}, {width}) {dt} tensor on {dev}")
        scratch = torch.empty(max(int(getattr(lib, scratch_entry)(B, width)), 2), dtype=torch.float32, device=dev)
        if a > 0.0:
            e = torch.empty(B, width, dtype=torch.float32, device=dev)
            N.check(lib.mvn_audio_frontend_emph(_AUDIO_FORMS[entry], pcm.data_ptr(), pcm.numel(),
                                                descriptors.data_ptr(), B, int(Q), int(width), int(bool(normalize)), a,
                                                y.data_ptr(), scratch.data_ptr(), idx.data_ptr(), e.data_ptr(),
                                                _stream_ptr(dev)), "mvn_audio_frontend_emph")
            return idx, y, e
        N.check(getattr(lib, entry)(pcm.data_ptr(), pcm.numel(), descriptors.data_ptr(), B, int(Q), int(width),
                                    int(bool(normalize)), y.data_ptr(), scratch.data_ptr(), idx.data_ptr(),
                                    _stream_ptr(dev)), entry)
    return idx, y, None


def _frontend_result(return_waveform: bool, idx, y, e):
    if not return_waveform:
        return idx
    return (idx, y) if e is None else (idx, y, e)


def audio_frontend(pcm: torch.Tensor, frames, channels, quantization_channels: int, n_out: int = None,
                   normalize: bool = True, offsets=None, descriptors: torch.Tensor = None,
                   return_waveform: bool = False, out: torch.Tensor = None, waveform_out: torch.Tensor = None,
                   preemphasis: float = 0.0):
    """Waveforms -> class indices on the GPU (mvn_audio_frontend): channel mean, resample of each whole clip to
    ``n_out`` frames (default MAX_AUDIO_FRAMES; sinc_interp_hann, width 6, roll-off 0.99), min-max normalisation,
    mu-law.

    ``pcm``: 1-D int16 tensor on the GPU, the clips' interleaved samples (8-bit files as ``(v - 128) << 8``, 24- and
    32-bit files rounded to 16 bits: dataset.read_wav_pcm16).  ``frames`` / ``channels`` / ``offsets``: per clip, host
    sequences (offsets default to back-to-back), checked here against the upload; ``descriptors`` is the same
    already on the device ((B, 4) int32 of audio_clip_descriptors -- the loader ships it through its pinned ring).
    Returns (B, n_out) int32 indices, with ``return_waveform`` also the (B, n_out) fp32 waveform before
    normalisation.  Nothing here waits for the GPU.

    ``preemphasis`` = a in (0, 1) (mvn_audio_frontend_emph; 0, the default, is the call above, untouched): what goes
    to mu-law is e[k] = (vn[k] - a vn[k-1]) / (1 + a) of the normalised row vn, vn[-1] = 0 -- the signal a model
    whose output is de-emphasised (``pcm16_chunk(deemphasis=a)``) trains on.  ``return_waveform`` then returns
    (indices, waveform, e)."""
    _check_pcm(pcm)  # (before the host lists are held against it)
    if n_out is None:
        from . import wavenet as W
        n_out = W.MAX_AUDIO_FRAMES
    B = len(frames)
    if B < 1 or len(channels) != B:
        raise ValueError("frames and channels must name the same, non-zero number of clips")
    desc = audio_clip_descriptors(frames, channels, offsets)
    rec = desc.view(_AUDIO_CLIP).reshape(B)
    for b in range(B):
        o, n, c = int(rec["offset"][b]), int(rec["frames"][b]), int(rec["channels"][b])
        if n < 1 or c < 1 or o < 0 or o + n * c > pcm.numel():
            raise ValueError(f"clip {b}: {n} frames x {c} channels at offset {o} do not lie inside the "
                             f"upload of {pcm.numel()} samples")
        if n > AUDIO_FRONTEND_MAX_RATIO * n_out:
            raise ValueError(f"clip {b}: {n} frames is more than {AUDIO_FRONTEND_MAX_RATIO} x the {n_out} "
                             "output frames the front end resamples to")
    if descriptors is None:
        descriptors = torch.from_numpy(desc).to(pcm.device)
    return _frontend_result(return_waveform, *_audio_frontend_call(
        "mvn_audio_frontend", "mvn_audio_frontend_scratch_floats", pcm, descriptors, 4, B, quantization_channels, n_out,
        normalize, waveform_out, out, preemphasis))


def audio_clip_var_descriptors(frames, channels, n_out, offsets=None):
    """Host array of mvn_audio_clip_var records (int64 offset, int32 frames, channels, n_out, reserved) as (B, 6)
    int32; ``offsets`` default to the clips lying back to back in the upload."""
    import numpy as np
    rec = np.zeros(len(frames), dtype=_AUDIO_CLIP_VAR)
    rec["frames"], rec["channels"], rec["n_out"] = frames, channels, n_out
    rec["offset"] = _back_to_back(rec["frames"].astype(np.int64) * rec["channels"], offsets)
    return rec.view(np.int32).reshape(len(frames), 6)


def audio_frontend_var(pcm: torch.Tensor, descriptors: torch.Tensor, quantization_channels: int, width: int,
                       normalize: bool = True, return_waveform: bool = False, preemphasis: float = 0.0):
    """Waveforms -> class indices by RATE (mvn_audio_frontend_var): clip b resampled as a whole to its own ``n_out``
    frames -- ``audio_frontend`` of that clip alone with that ``n_out``, bit for bit -- into row b of (B, ``width``)
    indices, silence (the class of 0.0) behind it.  ``descriptors``: (B, 6) int32 on the GPU
    (``audio_clip_var_descriptors``), checked on the device: a clip outside the upload or with ``n_out`` outside
    [1, width] gives a row of -1.  Nothing here waits for the GPU.  ``preemphasis``: as in ``audio_frontend``, over
    the row's own ``n_out`` columns; e is 0 behind them."""
    return _frontend_result(return_waveform, *_audio_frontend_call(
        "mvn_audio_frontend_var", "mvn_audio_frontend_var_scratch_floats", pcm, descriptors, 6, None,
        quantization_channels, width, normalize, preemphasis=preemphasis))


def audio_clip_window_descriptors(span_first, span_frames, file_frames, channels, out_first, n_out, rate_in, rate_out,
                                  lo=None, hi=None, offsets=None):
    """Host array of mvn_audio_clip_window records (64 bytes each: int64 offset, span_first, out_first, file_frames;
    int32 span_frames, channels, n_out, rate_in, rate_out; float32 lo, hi; int32 reserved) as (B, 16) int32.  One
    sequence per field (``rate_out`` may be one number); ``lo`` / ``hi`` default to 0, 0 -- the window's own range --
    and ``offsets`` to the spans lying back to back in the upload."""
    import numpy as np
    rec = np.zeros(len(span_frames), dtype=_AUDIO_CLIP_WINDOW)
    rec["span_first"], rec["span_frames"], rec["file_frames"] = span_first, span_frames, file_frames
    rec["channels"], rec["out_first"], rec["n_out"] = channels, out_first, n_out
    rec["rate_in"], rec["rate_out"] = rate_in, rate_out
    if lo is not None:
        rec["lo"] = lo
    if hi is not None:
        rec["hi"] = hi
    rec["offset"] = _back_to_back(rec["span_frames"].astype(np.int64) * rec["channels"], offsets)
    return rec.view(np.int32).reshape(len(span_frames), 16)


def audio_frontend_window(pcm: torch.Tensor, descriptors: torch.Tensor, quantization_channels: int, width: int,
                          normalize: bool = True, return_waveform: bool = False, preemphasis: float = 0.0):
    """Windows of files -> class indices by RATE (mvn_audio_frontend_window): row b is the columns ``[out_first,
    out_first + n_out)`` of its whole file's resample from ``rate_in`` to ``rate_out`` -- the bits this call gives for
    the whole file, cropped, which up to ``rate_in = 10 rate_out`` are ``audio_frontend_var``'s -- formed from the
    uploaded span alone, silence behind them.  With ``normalize``
    a descriptor's ``hi > lo`` is the range to normalise by (the loader's per-file gain), else the window's own
    (min, max).  ``descriptors``: (B, 16) int32 on the GPU (``audio_clip_window_descriptors``), checked on the device:
    a refused row (span outside the upload or not covering the window's taps, ``n_out`` outside [1, width], a window
    outside the file, rates or channels < 1) is -1.  Nothing here waits for the GPU.  ``preemphasis``: as in
    ``audio_frontend``; the WINDOW's first column has no predecessor (vn[-1] = 0), not the file's previous sample --
    a convention, so a window is no longer a crop of the whole file's emphasised row in its first column."""
    return _frontend_result(return_waveform, *_audio_frontend_call(
        "mvn_audio_frontend_window", "mvn_audio_frontend_window_scratch_floats", pcm, descriptors, 16, None,
        quantization_channels, width, normalize, preemphasis=preemphasis))


VIDEO_FRONTEND_SIZE = 64       # the front end's output is (64, 64) per frame (movenet/dataset.py:292-310)
VIDEO_FRONTEND_MAX_DIM = 4096  # H, W <= 4096: a gray source row fits the kernel's LDS row

_VIDEO_CLIP = [("offset", "<i8"), ("height", "<i4"), ("width", "<i4"), ("channels", "<i4"), ("reserved", "<i4")]


def video_clip_descriptors(shapes, n_frames: int, offsets=None):
    """Host array of mvn_video_clip records (int64 byte offset, int32 height, width, channels, reserved) as (B, 6)
    int32; ``shapes`` is one (H, W, channels) per clip and ``offsets`` default to the clips' ``n_frames`` frames lying
    back to back in the upload."""
    import numpy as np
    rec = np.zeros(len(shapes), dtype=_VIDEO_CLIP)
    if len(shapes):
        arr = np.asarray(shapes, dtype=np.int64).reshape(len(shapes), 3)
        rec["height"], rec["width"], rec["channels"] = arr[:, 0], arr[:, 1], arr[:, 2]
        rec["offset"] = _back_to_back(int(n_frames) * arr[:, 0] * arr[:, 1] * arr[:, 2], offsets)
    return rec.view(np.int32).reshape(len(shapes), 6)


def video_frontend(pix: torch.Tensor, shapes, n_frames: int, antialias: bool = False,
                   descriptors: torch.Tensor = None, *, offsets=None, out: torch.Tensor = None,
                   return_status: bool = False, check: bool = True):
    """Decoded frames -> 64 x 64 gray levels on the GPU (mvn_video_frontend): what the reference's loader does per
    frame, torchvision's ``rgb_to_grayscale`` then ``resize`` to (64, 64) (bilinear, ``antialias`` as given; False is
    what torchvision 0.13 - 0.16 do for tensors), rounded half to even.  No division by 255.

    ``pix``: 1-D uint8 tensor on the GPU, every clip's ``n_frames`` frames as (n_frames, H, W, channels) bytes.
    ``shapes``: per clip (H, W, channels), channels 3 (RGB) or 1 (already gray), H and W in [1, 4096]; ``offsets``:
    per clip, byte offsets into ``pix`` (default back to back); both are checked here against the upload.
    ``descriptors`` is the same already on the device ((B, 6) int32 of video_clip_descriptors -- the loader ships it
    through its pinned ring).  Returns the (B, n_frames, 64, 64) uint8 levels.  The kernel checks the descriptors it
    reads and reports per clip; a non-zero status raises ValueError (reading it waits for the launch), unless
    ``return_status`` asks for (levels, status) instead (the loader, which reads the status at the end of the epoch)
    or ``check=False`` skips the read.  The host checks see ``shapes`` and ``offsets`` only: a ``descriptors`` tensor
    that says something else is judged by the kernel alone, which keeps it memory-safe but reports through ``status``
    -- so with ``descriptors`` given, read the status."""
    import numpy as np
    _require_gpu(pix, "pix")
    if pix.dtype != torch.uint8 or pix.dim() != 1 or not pix.is_contiguous():
        raise ValueError("pix must be a contiguous 1-D uint8 tensor")
    if isinstance(n_frames, bool) or not isinstance(n_frames, (int, np.integer)) or n_frames < 1:
        raise ValueError(f"n_frames must be an integer >= 1, got {n_frames!r}")
    if antialias not in (False, True, 0, 1):
        raise ValueError(f"antialias must be False or True, got {antialias!r}")
    B, n = len(shapes), int(n_frames)
    if B < 1 or any(len(s) != 3 for s in shapes):
        raise ValueError("shapes must name a non-zero number of clips, one (H, W, channels) each")
    if offsets is not None and len(offsets) != B:
        raise ValueError("offsets must name the same number of clips as shapes")
    desc = video_clip_descriptors(shapes, n, offsets)
    rec = desc.view(_VIDEO_CLIP).reshape(B)
    for b in range(B):
        o, h, w, c = (int(rec[k][b]) for k in ("offset", "height", "width", "channels"))
        if c not in (1, 3):
            raise ValueError(f"clip {b}: {c} channels; frames are RGB (3) or gray (1)")
        if not (1 <= h <= VIDEO_FRONTEND_MAX_DIM and 1 <= w <= VIDEO_FRONTEND_MAX_DIM):
            raise ValueError(f"clip {b}: frames of {h} x {w} lie outside 1 .. {VIDEO_FRONTEND_MAX_DIM} per side")
        if o < 0 or o + n * h * w * c > pix.numel():
            raise ValueError(f"clip {b}: {n} frames of {h} x {w} x {c} at offset {o} do not lie inside the "
                             f"upload of {pix.numel()} bytes")
    dev = pix.device
    S = VIDEO_FRONTEND_SIZE
    with torch.cuda.device(dev):
        if descriptors is None:
            descriptors = torch.from_numpy(desc).to(dev)
        if (tuple(descriptors.shape) != (B, 6) or descriptors.dtype != torch.int32 or not descriptors.is_contiguous()
                or descriptors.device != dev):
            raise ValueError(f"descriptors must be a contiguous ({B}, 6) int32 tensor on {dev}")
        levels = out if out is not None else torch.empty(B, n, S, S, dtype=torch.uint8, device=dev)
        if (tuple(levels.shape) != (B, n, S, S) or levels.dtype != torch.uint8 or not levels.is_contiguous()
                or levels.device != dev):
            raise ValueError(f"out must be a contiguous ({B}, {n}, {S}, {S}) uint8 tensor on {dev}")
        status = torch.empty(B, dtype=torch.int32, device=dev)
        N.check(N.lib().mvn_video_frontend(pix.data_ptr(), pix.numel(), descriptors.data_ptr(), B, n,
                                           int(bool(antialias)), levels.data_ptr(), status.data_ptr(),
                                           _stream_ptr(dev)), "mvn_video_frontend")
    if return_status:
        return levels, status
    if check:
        st = status.cpu().tolist()
        if any(st):
            why = {1: "its span does not lie inside the upload", 2: "channels is not 1 or 3",
                   3: "height or width outside 1 .. 4096"}
            b = next(i for i, s in enumerate(st) if s)
            raise ValueError(f"mvn_video_frontend refused clip {b} on the device: {why.get(st[b], st[b])}")
    return levels


class _CrossEntropyOnProbs(torch.autograd.Function):
    """loss, accuracy of the trainer (row F3): mvn_ce_on_probs_forward / _backward."""

    @staticmethod
    def forward(ctx_, probs, target):
        _require_gpu(probs, "probs")
        if probs.dim() != 3 or target.shape != (probs.shape[0], probs.shape[2]):
            raise ValueError(f"probs (B,Q,S) / target (B,S) expected, got {tuple(probs.shape)} / "
                             f"{tuple(target.shape)}")
        p = probs.detach().to(torch.float32).contiguous()
        tg = target.detach().to(device=p.device, dtype=torch.int64).contiguous()
        B, Q, S = p.shape
        lib = N.lib()
        with torch.cuda.device(p.device):
            parts = lib.mvn_ce_parts(B, S)
            loss_part = torch.zeros(max(parts, 1), dtype=torch.float32, device=p.device)
            ok_part = torch.zeros(max(parts, 1), dtype=torch.int32, device=p.device)
            N.check(lib.mvn_ce_on_probs_forward(p.data_ptr(), tg.data_ptr(), B, Q, S, loss_part.data_ptr(),
                                                ok_part.data_ptr(), _stream_ptr(p.device)),
                    "mvn_ce_on_probs_forward")
        n = max(B * S, 1)
        ctx_.save_for_backward(p, tg)
        ctx_.in_dtype = probs.dtype
        loss = loss_part.sum() / n
        acc = ok_part.sum().to(torch.float32) / n
        ctx_.mark_non_differentiable(acc)
        return loss, acc

    @staticmethod
    def backward(ctx_, dloss, _dacc):
        p, tg = ctx_.saved_tensors
        B, Q, S = p.shape
        dp = torch.empty_like(p)
        up = dloss.detach().to(device=p.device, dtype=torch.float32).reshape(1).contiguous()
        with torch.cuda.device(p.device):
            N.check(N.lib().mvn_ce_on_probs_backward(p.data_ptr(), tg.data_ptr(), B, Q, S,
                                                     1.0 / max(B * S, 1), up.data_ptr(), dp.data_ptr(),
                                                     _stream_ptr(p.device)), "mvn_ce_on_probs_backward")
        return dp.to(ctx_.in_dtype), None


def cross_entropy_on_probs(probs: torch.Tensor, target: torch.Tensor):
    """(loss, accuracy) of movenet/pytorch_lightning_trainer.py:64-66 in two kernels:
    ``F.cross_entropy(probs, target)`` -- a log-softmax applied to what already are
    probabilities -- and ``(probs.argmax(1) == target).float().mean()``."""
    return _CrossEntropyOnProbs.apply(probs, target)


# ----------------------------------------------------------------------------------------------------------------
# The five building blocks as autograd nodes of their own (csrc/blocks.hip, mvn_block_*): what movenet_amd.modules'
# forward methods call.  fp32, (batch, channels, frames), contiguous; activations are saved only when a gradient is
# needed, and gradients come back as ordinary tensors (the flat buffers of _run_backward are the whole model's).
# ----------------------------------------------------------------------------------------------------------------
def _f32c(t):
    return None if t is None else t.detach().to(torch.float32).contiguous()


def _bt(t):
    """mvn_block_tensor of a contiguous (B, ch, len) tensor (or None)."""
    return None if t is None else N.BlockTensor(t.data_ptr(), t.stride(1), t.shape[2])


def _ptr(t):
    return None if t is None else t.data_ptr()


def _scratch(n: int, dev):
    n = int(n)
    return torch.empty(max(n, 1), dtype=torch.float32, device=dev), n


def _block_input(x, what: str, channels: int):
    if x.dim() != 3 or x.shape[1] != channels:
        raise ValueError(f"{what} must be (batch, {channels}, frames), got {tuple(x.shape)}")
    if x.shape[0] < 1 or x.shape[2] < 1:
        raise ValueError(f"{what} must not be empty, got {tuple(x.shape)}")


class _Conv2TapFunction(torch.autograd.Function):
    """CausalConv1d (dilation 0: taps t - 1 and t, same length) and DilatedCausalConv1d (taps j and j + d)."""

    @staticmethod
    def forward(ctx_, dilation, x, w, bias):
        lib = N.lib()
        x, w, bias = _f32c(x), _f32c(w), _f32c(bias)
        B, cin, T = x.shape
        cout = w.shape[0]
        n = T - dilation
        dev = x.device
        with torch.cuda.device(dev):
            y = torch.empty((B, cout, n), dtype=torch.float32, device=dev)
            if dilation == 0:
                N.check(lib.mvn_block_causal_forward(w.data_ptr(), _ptr(bias), cin, cout, _bt(x), _bt(y), B,
                                                     _stream_ptr(dev)), "mvn_block_causal_forward")
            else:
                N.check(lib.mvn_block_dilated_forward(w.data_ptr(), _ptr(bias), cin, dilation, _bt(x), _bt(y), B,
                                                      _stream_ptr(dev)), "mvn_block_dilated_forward")
        ctx_.dilation, ctx_.has_bias = dilation, bias is not None
        if any(ctx_.needs_input_grad):
            ctx_.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx_, dy):
        lib = N.lib()
        x, w = ctx_.saved_tensors
        B, cin, T = x.shape
        cout, d = w.shape[0], ctx_.dilation
        dev = x.device
        dy = _f32c(dy)
        need_x, need_w, need_b = ctx_.needs_input_grad[1], ctx_.needs_input_grad[2], ctx_.needs_input_grad[3] and ctx_.has_bias
        with torch.cuda.device(dev):
            dx = torch.empty_like(x) if need_x else None
            dw = torch.zeros_like(w) if need_w else None
            db = torch.zeros(cout, dtype=torch.float32, device=dev) if need_b else None
            scratch, ns = _scratch(lib.mvn_block_conv_scratch_floats(cin, cout, B, T - d), dev)
            if d == 0:
                N.check(lib.mvn_block_causal_backward(w.data_ptr(), cin, cout, _bt(x), _bt(dy), _bt(dx), _ptr(dw), _ptr(db),
                                                      B, scratch.data_ptr(), ns, _stream_ptr(dev)),
                        "mvn_block_causal_backward")
            else:
                N.check(lib.mvn_block_dilated_backward(w.data_ptr(), cin, d, _bt(x), _bt(dy), _bt(dx), _ptr(dw), _ptr(db),
                                                       B, scratch.data_ptr(), ns, _stream_ptr(dev)),
                        "mvn_block_dilated_backward")
        return None, dx, dw, db


# per-layer parameter order of the gated layer's nodes (biases of the dilated convs are None in the reference's layer)
GATED_PARAMS = ("filter_w", "filter_b", "gate_w", "gate_b", "ctx_filter_w", "ctx_filter_b", "ctx_gate_w", "ctx_gate_b",
                "residual_w", "residual_b", "skip_w", "skip_b")


def _gated_struct(tensors):
    return N.BlockGatedParams(*[_ptr(t) for t in tensors])


def _gated_forward_call(lib, ps, C, K, d, x, context, residual, skip, th, sg):
    dev = x.device
    B, T = x.shape[0], x.shape[2]
    ns = 0 if th is not None else int(lib.mvn_block_gated_scratch_floats(C, K, B, T, d, int(context is not None), 0))
    scratch, ns = _scratch(ns, dev)
    N.check(lib.mvn_block_gated_forward(_gated_struct(ps), C, K, d, _bt(x), _bt(context), _bt(residual), _bt(skip),
                                        _bt(th), _bt(sg), B, scratch.data_ptr(), ns, _stream_ptr(dev)),
            "mvn_block_gated_forward")


def _gated_backward_call(lib, ps, grads, C, K, d, x, context, th, sg, d_res, d_skip, dx, dctx):
    dev = x.device
    B, T = x.shape[0], x.shape[2]
    scratch, ns = _scratch(lib.mvn_block_gated_scratch_floats(C, K, B, T, d, int(context is not None), 1), dev)
    N.check(lib.mvn_block_gated_backward(_gated_struct(ps), _gated_struct(grads), C, K, d, _bt(x), _bt(context), _bt(th),
                                         _bt(sg), _bt(d_res), _bt(d_skip), _bt(dx), _bt(dctx), B, scratch.data_ptr(), ns,
                                         _stream_ptr(dev)), "mvn_block_gated_backward")


def _check_gated_shapes(x, context, C, d):
    _block_input(x, "input", C)
    T = x.shape[2]
    if T <= d:
        raise RuntimeError(f"dilated causal convolution: input length T = {T} does not exceed the dilation d = {d}")
    if context is not None:
        _block_input(context, "context", C)
        if context.shape[0] != x.shape[0]:
            raise ValueError(f"context batch {context.shape[0]} != input batch {x.shape[0]}")


class _GatedLayerFunction(torch.autograd.Function):
    """GatedResidualConv1d: (input, context) -> (residual (B,C,T-d), skip (B,K,s)); s columns, already resolved."""
    N_FIXED = 4

    @staticmethod
    def forward(ctx_, dilation, s, x, context, *params):
        lib = N.lib()
        x, context = _f32c(x), _f32c(context)
        ps = [_f32c(p) for p in params]
        C, K = ps[8].shape[0], ps[10].shape[0]
        B, _, T = x.shape
        n = T - dilation
        dev = x.device
        save = any(ctx_.needs_input_grad)
        ctx_.set_materialize_grads(False)  # an output nobody used arrives as None, not as a tensor of zeros
        with torch.cuda.device(dev):
            f32 = dict(dtype=torch.float32, device=dev)
            res, skip = torch.empty((B, C, n), **f32), torch.empty((B, K, s), **f32)
            th = torch.empty((B, C, n), **f32) if save else None
            sg = torch.empty((B, C, n), **f32) if save else None
            _gated_forward_call(lib, ps, C, K, dilation, x, context, res, skip, th, sg)
        ctx_.dilation, ctx_.has_context, ctx_.present = dilation, context is not None, [p is not None for p in ps]
        if save:
            ctx_.save_for_backward(x, th, sg, *([context] if context is not None else []), *[p for p in ps if p is not None])
        return res, skip

    @staticmethod
    def backward(ctx_, d_res, d_skip):
        if d_res is None and d_skip is None:
            return (None,) * (_GatedLayerFunction.N_FIXED + len(ctx_.present))
        lib = N.lib()
        x, th, sg, *rest = ctx_.saved_tensors
        context = rest.pop(0) if ctx_.has_context else None
        it = iter(rest)
        ps = [next(it) if here else None for here in ctx_.present]
        C, K, d = ps[8].shape[0], ps[10].shape[0], ctx_.dilation
        dev = x.device
        need = ctx_.needs_input_grad
        with torch.cuda.device(dev):
            d_res, d_skip = _f32c(d_res), _f32c(d_skip)
            dx = torch.empty_like(x) if need[2] else None
            dctx = torch.empty_like(context) if (context is not None and need[3]) else None
            grads = []
            for i, p in enumerate(ps):
                ctx_only = 4 <= i < 8
                want = p is not None and need[_GatedLayerFunction.N_FIXED + i] and (context is not None or not ctx_only)
                want = want and not (i in (8, 9) and d_res is None) and not (i in (10, 11) and d_skip is None)
                grads.append(torch.zeros_like(p) if want else None)
            _gated_backward_call(lib, ps, grads, C, K, d, x, context, th, sg, d_res, d_skip, dx, dctx)
        return (None, None, dx, dctx, *grads)


class _ResidualStackFunction(torch.autograd.Function):
    """ResidualConvStack: the layers in turn; layer l writes its skip into plane l of the (L, B, K, s) result."""
    N_FIXED = 4

    @staticmethod
    def forward(ctx_, dilations, s, x, context, *params):
        lib = N.lib()
        x, context = _f32c(x), _f32c(context)
        ps = [_f32c(p) for p in params]
        L, P = len(dilations), len(GATED_PARAMS)
        C, K = ps[8].shape[0], ps[10].shape[0]
        B = x.shape[0]
        dev = x.device
        save = any(ctx_.needs_input_grad)
        saved = []
        with torch.cuda.device(dev):
            f32 = dict(dtype=torch.float32, device=dev)
            skips = torch.empty((L, B, K, s), **f32)
            cur = x
            for l, d in enumerate(dilations):
                n = cur.shape[2] - d
                res = torch.empty((B, C, n), **f32)
                th = torch.empty((B, C, n), **f32) if save else None
                sg = torch.empty((B, C, n), **f32) if save else None
                _gated_forward_call(lib, ps[l * P:(l + 1) * P], C, K, d, cur, context, res, skips[l], th, sg)
                if save:
                    saved += [cur, th, sg]
                cur = res
        ctx_.dilations, ctx_.has_context, ctx_.present = dilations, context is not None, [p is not None for p in ps]
        if save:
            ctx_.save_for_backward(*saved, *([context] if context is not None else []), *[p for p in ps if p is not None])
        return skips

    @staticmethod
    def backward(ctx_, d_skips):
        lib = N.lib()
        dil = ctx_.dilations
        L, P = len(dil), len(GATED_PARAMS)
        tensors = list(ctx_.saved_tensors)
        acts, rest = tensors[:3 * L], tensors[3 * L:]
        context = rest.pop(0) if ctx_.has_context else None
        it = iter(rest)
        ps = [next(it) if here else None for here in ctx_.present]
        C, K = ps[8].shape[0], ps[10].shape[0]
        need = ctx_.needs_input_grad
        dev = acts[0].device
        grads = [None] * len(ps)
        with torch.cuda.device(dev):
            d_skips = _f32c(d_skips)
            want_ctx = context is not None and need[3]
            dctx = torch.zeros_like(context) if want_ctx else None
            dctx_l = torch.empty_like(context) if want_ctx else None
            d_res = None  # the last layer's residual leaves the stack unused (movenet/modules.py:119-130)
            for l in reversed(range(L)):
                x, th, sg = acts[3 * l:3 * l + 3]
                lp = ps[l * P:(l + 1) * P]
                lg = []
                for i, p in enumerate(lp):
                    want = p is not None and need[_ResidualStackFunction.N_FIXED + l * P + i]
                    want = want and (context is not None or not 4 <= i < 8) and not (i in (8, 9) and d_res is None)
                    lg.append(torch.zeros_like(p) if want else None)
                dx = torch.empty_like(x) if (l > 0 or need[2]) else None
                _gated_backward_call(lib, lp, lg, C, K, dil[l], x, context, th, sg, d_res, d_skips[l], dx, dctx_l)
                if want_ctx:
                    dctx += dctx_l
                grads[l * P:(l + 1) * P] = lg
                d_res = dx
        return (None, None, d_res if need[2] else None, dctx, *grads)


class _DenseConvFunction(torch.autograd.Function):
    """DenseConv: conv2(leaky_relu(conv1(leaky_relu(x)))); the hidden layer is saved only when a gradient is needed."""

    @staticmethod
    def forward(ctx_, x, w1, b1, w2, b2):
        lib = N.lib()
        x, w1, b1, w2, b2 = (_f32c(t) for t in (x, w1, b1, w2, b2))
        B, K, S = x.shape
        Q = w1.shape[0]
        dev = x.device
        save = any(ctx_.needs_input_grad)
        with torch.cuda.device(dev):
            f32 = dict(dtype=torch.float32, device=dev)
            y = torch.empty((B, Q, S), **f32)
            h = torch.empty((B, Q, S), **f32) if save else None
            scratch, ns = _scratch(0 if save else lib.mvn_block_dense_scratch_floats(K, Q, B, S, 0), dev)
            N.check(lib.mvn_block_dense_forward(w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), K, Q, _bt(x),
                                                _bt(h), _bt(y), B, scratch.data_ptr(), ns, _stream_ptr(dev)),
                    "mvn_block_dense_forward")
        if save:
            ctx_.save_for_backward(x, h, w1, w2)
        return y

    @staticmethod
    def backward(ctx_, dy):
        lib = N.lib()
        x, h, w1, w2 = ctx_.saved_tensors
        B, K, S = x.shape
        Q = w1.shape[0]
        dev = x.device
        need = ctx_.needs_input_grad
        with torch.cuda.device(dev):
            dy = _f32c(dy)
            dx = torch.empty_like(x) if need[0] else None
            dw1 = torch.zeros_like(w1) if need[1] else None
            db1 = torch.zeros(Q, dtype=torch.float32, device=dev) if need[2] else None
            dw2 = torch.zeros_like(w2) if need[3] else None
            db2 = torch.zeros(Q, dtype=torch.float32, device=dev) if need[4] else None
            scratch, ns = _scratch(lib.mvn_block_dense_scratch_floats(K, Q, B, S, 1), dev)
            N.check(lib.mvn_block_dense_backward(w1.data_ptr(), w2.data_ptr(), K, Q, _bt(x), _bt(h), _bt(dy), _bt(dx),
                                                 _ptr(dw1), _ptr(db1), _ptr(dw2), _ptr(db2), B, scratch.data_ptr(), ns,
                                                 _stream_ptr(dev)), "mvn_block_dense_backward")
        return dx, dw1, db1, dw2, db2


def block_causal_conv(x, weight, bias=None):
    _block_input(x, "input", weight.shape[1])
    return _Conv2TapFunction.apply(0, x, weight, bias)


def block_dilated_conv(x, weight, bias, dilation: int):
    _block_input(x, "input", weight.shape[1])
    if x.shape[2] <= dilation:
        raise RuntimeError(f"dilated causal convolution: input length T = {x.shape[2]} does not exceed the dilation "
                           f"d = {dilation}")
    return _Conv2TapFunction.apply(int(dilation), x, weight, bias)


def _resolved_context(context, n: int):
    if context is not None and context.shape[2] < n:
        raise ValueError(f"context has {context.shape[2]} columns, the layer's output has T - d = {n}")
    return context


def block_gated_layer(x, context, skip_size: int, dilation: int, params):
    """``params``: the twelve tensors of GATED_PARAMS (None where the layer has no such bias)."""
    C = params[8].shape[0]
    _check_gated_shapes(x, context, C, dilation)
    skip_size = int(skip_size)
    if skip_size < 0:
        raise ValueError(f"skip_size must not be negative, got {skip_size}")
    n = x.shape[2] - dilation
    _resolved_context(context, n)
    s = n if (skip_size == 0 or skip_size > n) else skip_size  # skip[:, :, -skip_size:]
    return _GatedLayerFunction.apply(int(dilation), s, x, context, *params)


def block_residual_stack(x, context, skip_size: int, dilations, layer_params):
    """``layer_params``: one GATED_PARAMS list per layer.  Returns the (L, B, K, skip_size) stack of skips."""
    C = layer_params[0][8].shape[0]
    _block_input(x, "input", C)
    skip_size = int(skip_size)
    out_len = x.shape[2] - sum(dilations)
    if not 1 <= skip_size <= out_len:
        raise ValueError(f"skip_size must lie in [1, T - sum(dilations)] = [1, {out_len}], got {skip_size}")
    if context is not None:
        _block_input(context, "context", C)
        if context.shape[0] != x.shape[0] or context.shape[2] != x.shape[2]:
            raise ValueError(f"context must be aligned with the input, (batch, {C}, {x.shape[2]}); got "
                             f"{tuple(context.shape)}")
    flat = [p for lp in layer_params for p in lp]
    return _ResidualStackFunction.apply(tuple(int(d) for d in dilations), skip_size, x, context, *flat)


def block_dense_conv(x, w1, b1, w2, b2):
    _block_input(x, "input", w1.shape[1])
    return _DenseConvFunction.apply(x, w1, b1, w2, b2)
