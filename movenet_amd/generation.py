"""Host side of the ring-buffer generator: owns the packed weights, the
dilation-queue state and the sample buffer as torch tensors (device memory and
stream plumbing only) and drives ``mvn_generate_trunc`` -- or, with settings per sequence,
``mvn_generate_seq`` -- through the C ABI.

Replaces the per-sample window loop of /root/reference/movenet/wavenet.py:217-237.
"""
from __future__ import annotations

import threading

import os
from typing import Dict, Optional

import torch

from . import _native as N


class PipeHandoffTimeout(RuntimeError):
    """A stage of the PIPE generator waited for its predecessor beyond the spin bound: its
    workgroups were not co-resident (another process or stream held CUs).  The samples of
    that call are NOT valid."""


def wait_event(event, spin_s: float = 5.0) -> None:
    """Host wait for a recorded torch.cuda.Event by polling it (a core polling for the few
    milliseconds of a step costs nothing that matters: one process drives one GPU)."""
    import time
    t0 = time.perf_counter()
    spins = 0
    while not event.query():
        spins += 1
        if spins > 200:
            time.sleep(20e-6)
            if time.perf_counter() - t0 > spin_s:
                event.synchronize()
                return


class HostWords:
    """Device scalars read by the host WITHOUT a stream synchronisation, a second stream or a copy
    engine (``mvn_publish_words``): a ring of slots in pinned, device-visible host memory per
    device; a one-wave kernel queued on the producing stream writes up to 64 32-bit words and then
    a sequence number the host polls for.  ``publish`` returns a token, ``read`` spins on it.

    ``tensor.item()`` waits for everything enqueued on the stream so far -- read in the middle of a
    training step it would serialise the host's enqueueing with the GPU's execution.  Here the host
    waits exactly for the kernels in front of the publish kernel (the one-hot check of
    WaveNet.forward, published BEFORE the forward is enqueued; the trainer's log scalars, read one
    step late)."""
    RING, MAXW = 16, 64
    _rings: dict = {}
    _lock = threading.Lock()

    @classmethod
    def publish(cls, words: torch.Tensor):
        """``words``: 1-D device tensor of <= 64 int32 / float32 values (already computed or being
        computed on the current stream).  Returns the token ``read`` takes.  Thread-safe; when the
        ring wraps onto a slot whose token has not been read yet, that token is RESOLVED first (its
        values are copied out of the slot into the token), so a 17th publish never overwrites
        values somebody is still going to ask for."""
        n = int(words.numel())
        if not 1 <= n <= cls.MAXW or words.dtype not in (torch.int32, torch.float32) or not words.is_contiguous():
            raise ValueError("HostWords.publish: 1..64 contiguous int32 / float32 values")
        dev = words.device
        key = dev.index if dev.index is not None else torch.cuda.current_device()
        with cls._lock:
            ring = cls._rings.get(key)
            if ring is None:
                ring = cls._rings[key] = [torch.zeros(cls.RING, cls.MAXW + 1, dtype=torch.int32).pin_memory(), 0,
                                          [None] * cls.RING]
            ring[1] += 1
            seq = (ring[1] & 0x3FFFFFFF) or 1
            at = ring[1] % cls.RING
            slot = ring[0][at]
            old = ring[2][at]
            if old is not None and old[4][0] is None:  # outstanding: wait for it, keep its values in the token
                old[4][0] = cls._wait(old)
            token = (slot, n, seq, words, [None])  # (words kept alive until read; [4]: values once resolved)
            ring[2][at] = token
            with torch.cuda.device(dev):
                N.check(N.lib().mvn_publish_words(words.data_ptr(), n, seq, slot.data_ptr(),
                                                  torch.cuda.current_stream(dev).cuda_stream), "mvn_publish_words")
        return token

    @staticmethod
    def _wait(token, timeout_s: float = 30.0):
        import time
        slot, n, seq, words, _ = token
        t0 = time.perf_counter()
        spins = 0
        while int(slot[n]) != seq:
            spins += 1
            if spins > 200:
                # (a read that is not there after ~100 us is waiting for milliseconds of GPU work that
                # the caller has overlapped with its own: yield the core between polls -- eight ranks
                # of a node spinning flat out would eat eight cores of the container's quota)
                time.sleep(20e-6)
                if time.perf_counter() - t0 > timeout_s:  # (never seen: the blocking form as a last resort)
                    return words.tolist()
        vals = slot[:n]
        return vals.tolist() if words.dtype == torch.int32 else vals.view(torch.float32).tolist()

    @classmethod
    def read(cls, token, timeout_s: float = 30.0):
        """The published values as a list of Python ints / floats (by the dtype of ``words``)."""
        with cls._lock:  # (against a publish that wraps onto this token's slot at the same moment)
            if token[4][0] is None:
                token[4][0] = cls._wait(token, timeout_s)
        return token[4][0]


def _stream_ptr(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _require_gpu(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(
            f"movenet_amd: {what} must live on an MI355X device (got {t.device}); "
            "there is no CPU path in this package"
        )


def pack_params(dims: N.Dims, sd: Dict[str, torch.Tensor], n_layers: int):
    """Build the mvn_params struct from a state_dict of fp32 device tensors.
    Returns (struct, keepalive) -- keepalive holds the pointer arrays and the
    contiguous tensors the struct points into."""
    keep = []

    def dev(key: str) -> int:
        t = sd[key]
        _require_gpu(t, key)
        if t.dtype != torch.float32:
            raise TypeError(f"{key}: expected float32, got {t.dtype}")
        t = t.detach().contiguous()
        keep.append(t)
        return t.data_ptr()

    def per_layer(name: str):
        ptrs = [dev(f"residual_conv_stack.conv_layers.{l}.{name}") for l in range(n_layers)]
        arr, cast = N.ptr_array(ptrs)
        keep.append(arr)
        return cast

    p = N.Params()
    p.causal_w = dev("causal_conv.conv.weight")
    p.filter_w = per_layer("conv_filter.conv.weight")
    p.gate_w = per_layer("conv_gate.conv.weight")
    p.residual_w = per_layer("conv_residual.weight")
    p.residual_b = per_layer("conv_residual.bias")
    p.skip_w = per_layer("conv_skip.weight")
    p.skip_b = per_layer("conv_skip.bias")
    has_ctx = "residual_conv_stack.conv_layers.0.context_conv_filter.weight" in sd
    if has_ctx:
        p.ctx_filter_w = per_layer("context_conv_filter.weight")
        p.ctx_filter_b = per_layer("context_conv_filter.bias")
        p.ctx_gate_w = per_layer("context_conv_gate.weight")
        p.ctx_gate_b = per_layer("context_conv_gate.bias")
    p.head1_w = dev("dense_conv.conv1.weight")
    p.head1_b = dev("dense_conv.conv1.bias")
    p.head2_w = dev("dense_conv.conv2.weight")
    p.head2_b = dev("dense_conv.conv2.bias")
    return p, keep


class ContextSource:
    """What a generator with a WINDOWED context reads its conditioning from: the frame-rate rows and / or
    the label's vectors, a few hundred kilobytes where the two whole-context tensors take 8 C bytes per generated column
    and row.  ``RingGenerator(context_source=...)`` forms the columns of each launch from it (``ops.context_window``).

    ``proj``: (batch, C, F) fp32 on the device from ``ops.project_features``, frames ``hop`` samples apart, or None;
    ``glob``: (batch, C) fp32, one vector per sequence, or None (not both None);
    ``prompt``: with ``proj``, a callable P -> the (batch, C, P) channel-major local context of columns [0, P), as
    ``ops.upsample_features(model, feats, P)`` forms it from ALL the frames -- ``prime()`` runs the prompt's forward
    pass on it."""

    def __init__(self, proj: Optional[torch.Tensor] = None, hop: int = 0, glob: Optional[torch.Tensor] = None,
                 prompt=None):
        if proj is None and glob is None:
            raise ValueError("ContextSource: proj and glob are both None (an unconditioned generator takes no source)")
        if proj is not None:
            _require_gpu(proj, "ContextSource.proj")
            if proj.dim() != 3 or proj.dtype != torch.float32:
                raise ValueError(f"proj must be (batch, C, frames) float32, got {tuple(proj.shape)} {proj.dtype}")
            if isinstance(hop, bool) or not isinstance(hop, int) or hop < 1:
                raise ValueError(f"hop must be an integer >= 1, got {hop!r}")
            if prompt is None:
                raise ValueError("ContextSource: proj needs prompt, the callable that forms the prompt's columns")
            proj = proj.detach().contiguous()
        if glob is not None:
            _require_gpu(glob, "ContextSource.glob")
            if glob.dim() != 2 or (proj is not None and (glob.shape[0] != proj.shape[0] or glob.shape[1] != proj.shape[1])):
                raise ValueError(f"glob must be (batch, C), got {tuple(glob.shape)}")
            glob = glob.detach().to(torch.float32).contiguous()
        self.proj, self.hop, self.glob, self.prompt = proj, int(hop), glob, prompt

    @property
    def batch(self) -> int:
        return int((self.proj if self.proj is not None else self.glob).shape[0])

    @property
    def channels(self) -> int:
        return int((self.proj if self.proj is not None else self.glob).shape[1])

    def columns(self) -> Optional[int]:
        """How many columns the frames cover (None: any number, a label alone)."""
        return None if self.proj is None else int(self.proj.shape[2]) * self.hop

    def rows(self, b0: int, b1: int) -> "ContextSource":
        """The source of sequences [b0, b1) (``GroupedGenerator``'s groups)."""
        prompt = self.prompt
        return ContextSource(None if self.proj is None else self.proj[b0:b1], self.hop,
                             None if self.glob is None else self.glob[b0:b1],
                             None if prompt is None else (lambda P: prompt(P)[b0:b1]))


class RingGenerator:
    """One batch of sequences being generated on one GPU.

    >>> g = RingGenerator(cfg, state_dict, batch=16, n_total=19072, device="cuda:0")
    >>> g.prime(prompt_idx)            # (B, RF) int class indices
    >>> g.advance(16000)               # 16000 new samples per sequence
    >>> g.samples                      # (B, n_total) int32
    """

    def __init__(self, layer_size: int, stack_size: int, input_channels: int,
                 residual_channels: int, skip_channels: int, state_dict: Dict[str, torch.Tensor],
                 batch: int, n_total: int, device, variant: int = N.GEN_AUTO,
                 temperature: float = 0.0, seed: int = 0,
                 context: Optional[torch.Tensor] = None, sampling: str = "reference", top_k: int = 0,
                 top_p: float = 1.0, rows=None, global_context: Optional[torch.Tensor] = None, guidance=None,
                 context_source: Optional[ContextSource] = None):
        """``context_source``: a ``ContextSource`` in place of ``context`` and ``global_context`` (giving
        it with either is a ValueError).  Nothing of n_total columns is built: ``context`` and ``context_tm`` stay None,
        every launch forms its own columns [t_begin, t_end) in one buffer on the generator's stream
        (``ops.context_window``; a label alone: filled once, re-based per launch) and goes through
        ``mvn_generate_windowed``.  The stream's order protects the buffer: the next window is written behind the launch
        that read the last.  Samples, logits and choices are those of the whole-context generator to the bit;
        ``teacher_forced`` is the whole-context generator's.
        ``guidance`` (classifier-free guidance): None (off), one scale or a sequence of ``batch``
        scales.  The generator then owns 2 * batch rows -- ``samples_all``: rows [0, batch) the unconditional ones,
        WITHOUT ``global_context`` (the zero vector in its place), rows [batch, 2 batch) the conditional ones with it;
        both with the same prompt, the same ``context`` and the caller's per-sequence settings (``rows`` included) --
        and launches ``mvn_generate_guided``; ``samples`` and ``teacher_forced`` expose the ``batch`` conditional rows.
        ``global_context``: (batch, C) fp32 on the device, one vector per sequence that conditions every step (global
        conditioning): added to every time row of the time-major context copy the kernels read
        (mvn_context_add_global); without ``context`` the copy is filled with it.  ``state_dict`` must then hold the
        layers' context convs.
        ``sampling``: what a sampled step (temperature > 0) draws from -- "reference": the reference's
        softmax(softmax(logits) / T), close to uniform whatever the model predicts; "model": the model's own
        softmax(logits / T).  Greedy decoding (temperature <= 0) is the same under both.
        ``top_k`` / ``top_p``: truncation of a sampled step before the draw (include/movenet_hip.h,
        mvn_generate_trunc) -- keep the ``top_k`` likeliest classes (0: off), then the smallest head of them that holds
        ``top_p`` of their mass (1.0: off); greedy decoding ignores both.
        ``temperature``, ``seed``, ``top_k`` and ``top_p`` each take one value or a sequence / 1-D tensor of ``batch``
        values.  All four single: one ``mvn_generate_trunc`` launch with them, sequence b drawing on Philox row b.  Any
        of them a sequence (or ``rows`` given): the settings go to the device once and the launches are
        ``mvn_generate_seq``'s -- sequence b samples by its own entry, on its own seed and on row ``rows[b]``
        (default b), so its draws do not depend on where in which batch it sits.  The attributes are then lists."""
        self._sampling = N.sampling_rule(sampling)
        self.sampling = sampling
        if context_source is not None:
            if context is not None or global_context is not None:
                raise ValueError("context_source replaces context and global_context: give one or the other")
            if context_source.batch != int(batch) or context_source.channels != int(residual_channels):
                raise ValueError(f"context_source must hold ({int(batch)}, {int(residual_channels)}, ...) rows, got "
                                 f"({context_source.batch}, {context_source.channels}, ...)")
            cover = context_source.columns()
            if cover is not None and (int(n_total) - 1) // context_source.hop + 1 > cover // context_source.hop:
                raise ValueError(f"context_source holds {cover // context_source.hop} frames; {int(n_total)} samples at "
                                 f"hop {context_source.hop} need {(int(n_total) - 1) // context_source.hop + 1}")
        self.guidance = None if guidance is None else N.guidance_scales(batch, guidance)  # ValueError before anything is allocated
        guided = self.guidance is not None
        seq_host = None
        if guided or rows is not None or N.any_per_sequence(temperature, seed, top_k, top_p):  # ValueError before anything is allocated
            seq_host = N.seq_sampling_array(batch, input_channels, temperature, top_k, top_p, seed, rows)
            entries = [seq_host[b] for b in range(int(batch))]
            temperature, seed = [e.temperature for e in entries], [e.seed for e in entries]
            self.top_k, self.top_p = [e.top_k for e in entries], [e.top_p for e in entries]
            self.rows = [e.row for e in entries]
            if guided:  # the pair's two rows sample by the same entry (the kernel reads the conditional row's)
                both = (N.SeqSampling * (2 * int(batch)))()
                for b, e in enumerate(entries):
                    both[b] = both[b + int(batch)] = e
                seq_host = both
        else:
            self.top_k, self.top_p = N.truncation(top_k, top_p)
            temperature, seed = float(temperature), int(seed) & (2 ** 64 - 1)
        self.lib = N.lib()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("movenet_amd.RingGenerator needs an MI355X device; no CPU path exists")
        self.dims = N.make_dims(layer_size, stack_size, input_channels, residual_channels,
                                skip_channels)
        self.n_layers = layer_size * stack_size
        self.Q = input_channels
        self.rf = N.check(self.lib.mvn_receptive_fields(self.dims), "mvn_receptive_fields")
        self.batch, self.n_total = int(batch), int(n_total)
        self.nrows = 2 * self.batch if guided else self.batch  # rows of state, samples and context the launches see
        with torch.cuda.device(self.device):
            if guided and variant == N.GEN_AUTO:  # the best kernel with a guided form that holds the pairs
                variant = next((v for v in (N.GEN_FOLD, N.GEN_PIPE, N.GEN_GENERIC)
                                if self.lib.mvn_gen_guided_max_pairs(self.dims, v) >= self.batch
                                and self.lib.mvn_gen_variant(self.dims, v, self.nrows) == v), N.GEN_GENERIC)
            self.variant = N.check(self.lib.mvn_gen_variant(self.dims, variant, self.nrows),
                                   "mvn_gen_variant")
            if guided:
                limit = N.guided_max_pairs(self.dims, self.variant)
                if self.batch > limit:
                    raise RuntimeError(f"movenet_amd: a guided launch of variant {self.variant} takes at most {limit} "
                                       f"pairs for these dims ({self.batch} asked for)")
        if guided:  # the same video for both rows of a pair; the label's vector for the conditional rows only
            if context is not None:
                context = torch.cat([context, context], 0)
            if global_context is not None:
                if tuple(global_context.shape) != (batch, residual_channels):
                    raise ValueError(f"global_context must be (batch, {residual_channels}), got {tuple(global_context.shape)}")
                global_context = torch.cat([torch.zeros_like(global_context), global_context], 0)
        batch = self.nrows  # (r4: STREAM takes local conditioning too -- the context terms of all layers are formed at the top of a step)
        self.context = None      # (B, C, >= n_total) upsampled video as given
        self.context_tm = None   # (B, n_total, C) time-major copy the kernels read
        if context is not None:
            _require_gpu(context, "context")
            if context.shape[0] != batch or context.shape[1] != residual_channels or \
                    context.shape[2] < n_total:
                raise ValueError(f"context must be (batch, {residual_channels}, >= n_total), "
                                 f"got {tuple(context.shape)}")
            self.context = context.detach().to(torch.float32).contiguous()
            with torch.cuda.device(self.device):
                self.context_tm = torch.empty(self.nrows, self.n_total, residual_channels,
                                              dtype=torch.float32, device=self.device)
                N.check(self.lib.mvn_transpose_context(
                    self.context.data_ptr(), self.context.stride(1), self.nrows, residual_channels,
                    self.n_total, self.context_tm.data_ptr(), _stream_ptr(self.device)),
                    "mvn_transpose_context")
        self.global_context = None
        if global_context is not None:
            _require_gpu(global_context, "global_context")
            if tuple(global_context.shape) != (batch, residual_channels):
                raise ValueError(f"global_context must be (batch, {residual_channels}), got {tuple(global_context.shape)}")
            self.global_context = global_context.detach().to(torch.float32).contiguous()
            with torch.cuda.device(self.device):
                fill = self.context_tm is None
                if fill:
                    self.context_tm = torch.empty(self.nrows, self.n_total, residual_channels,
                                                  dtype=torch.float32, device=self.device)
                N.check(self.lib.mvn_context_add_global(
                    self.context_tm.data_ptr(), self.global_context.data_ptr(), self.nrows, residual_channels,
                    self.n_total, int(fill), _stream_ptr(self.device)), "mvn_context_add_global")
        # windowed context: the source, the label's vectors of ALL rows (guided: zeros in the unconditional ones, as
        # above) and the one window buffer; _win_cols: the columns a label-only buffer was filled for
        self._source, self._win, self._win_cols = context_source, None, 0
        if context_source is not None:
            _require_gpu(context_source.proj if context_source.proj is not None else context_source.glob, "context_source")
            g = context_source.glob
            if g is not None and guided:
                g = torch.cat([torch.zeros_like(g), g], 0)
            self.global_context = g
        self.temperature, self.seed = temperature, seed
        self._per_seq = None  # device copy of the mvn_seq_sampling array (per-sequence settings only)
        self._guidance = None  # device copy of the scales, one per pair (guided only)
        with torch.cuda.device(self.device):
            if seq_host is not None:
                self._per_seq = torch.frombuffer(seq_host, dtype=torch.uint8).to(self.device)
            if guided:
                self._guidance = torch.tensor(self.guidance, dtype=torch.float32).to(self.device)
            nw = self.lib.mvn_gen_weights_floats(self.dims, self.variant)
            ns = self.lib.mvn_gen_state_floats(self.dims, self.nrows)
            self._queue_floats = self.nrows * (self.rf - stack_size) * residual_channels
            # (MOVENET_DEBUG_GUARD=1, tests: a band of sentinels behind the packed weights and the state -- queues,
            # hand-off granules, placement words -- checked in check_errors())
            self._guard = None
            if os.environ.get("MOVENET_DEBUG_GUARD") == "1":
                band, sentinel = 1 << 16, -1234.5
                raw_p = torch.empty(nw + band, dtype=torch.float32, device=self.device)
                raw_s = torch.zeros(max(ns, 1) + band, dtype=torch.float32, device=self.device)
                raw_p[nw:].fill_(sentinel)
                raw_s[max(ns, 1):].fill_(sentinel)
                self.packed, self.state = raw_p[:nw], raw_s[:max(ns, 1)]
                self._guard = (sentinel, raw_p[nw:], raw_s[max(ns, 1):])
            else:
                self.packed = torch.empty(nw, dtype=torch.float32, device=self.device)
                self.state = torch.zeros(max(ns, 1), dtype=torch.float32, device=self.device)
            self.samples_all = torch.zeros(self.nrows, self.n_total, dtype=torch.int32, device=self.device)
        self.t = 0          # number of time steps consumed so far
        self.n_given = 1
        # queues primed by one full-sequence forward (MFMA kernels) instead of stepping; the
        # fp16-operand variant primes with the fp16-operand forward: ONE arithmetic throughout
        self.prime_with_forward = True
        self.repack(state_dict)

    @property
    def samples(self) -> torch.Tensor:
        """(batch, n_total) int32: every row the launches see -- guided: the conditional rows of ``samples_all``."""
        return self.samples_all[self.nrows - self.batch:]

    @samples.setter
    def samples(self, value: torch.Tensor) -> None:  # (GroupedGenerator: a row block of its shared tensor)
        if self._guidance is not None:
            raise RuntimeError("movenet_amd: the samples of a guided generator are a view of samples_all")
        self.samples_all = value

    def repack(self, state_dict: Dict[str, torch.Tensor]) -> None:
        self._sd = state_dict
        params, keep = pack_params(self.dims, state_dict, self.n_layers)
        with torch.cuda.device(self.device):
            N.check(self.lib.mvn_gen_pack_weights(self.dims, self.variant, params,
                                                  self.packed.data_ptr(), _stream_ptr(self.device)),
                    "mvn_gen_pack_weights")
        # the source tensors must outlive the enqueued pack kernels
        torch.cuda.current_stream(self.device).synchronize()
        del keep

    def reset(self) -> None:
        self.state.zero_()
        self.t = 0

    def status_word(self) -> Optional[torch.Tensor]:
        """The PIPE variant's sticky status word (a 1-element int32 view into the state), or
        None.  Non-zero since the last ``reset()`` = a hand-off timed out; every later launch
        is then a no-op until the state is zeroed again."""
        if self.variant not in N.PIPE_VARIANTS:
            return None
        word = self.lib.mvn_gen_status_offset(self.dims, self.nrows)
        return self.state[word:word + 1].view(torch.int32)

    def check_errors(self) -> None:
        """Synchronise and raise ``PipeHandoffTimeout`` if a PIPE hand-off timed out since
        the last ``reset()`` (workgroups of a pipeline not co-resident, e.g. another process
        occupying CUs).  Every product path calls this before handing samples on."""
        torch.cuda.current_stream(self.device).synchronize()
        if getattr(self, "_guard", None) is not None:
            sentinel, *bands = self._guard
            for band in bands:
                if bool((band != sentinel).any().item()):
                    raise RuntimeError("movenet_amd: a generator kernel wrote past the end of its packed weights / state")
        word = self.status_word()
        if word is not None and int(word[0].item()) != 0:
            raise PipeHandoffTimeout(
                "movenet_amd: PIPE generator hand-off timed out (pipeline stages not "
                "co-resident); the samples of this call are not valid")

    def _run(self, t_begin: int, t_end: int, n_given: int, logits_out=None, choices_out=None,
             logits_t0: int = 0) -> None:
        if self._source is not None:
            return self._run_windowed(t_begin, t_end, n_given, logits_out, choices_out, logits_t0)
        if self._guidance is not None:
            with torch.cuda.device(self.device):
                N.check(self.lib.mvn_generate_guided(
                    self.dims, self.variant, self.packed.data_ptr(), self.state.data_ptr(),
                    self.samples_all.data_ptr(), self.batch, self.samples_all.stride(0), self.n_total, n_given,
                    t_begin, t_end, self._per_seq.data_ptr(), self._guidance.data_ptr(),
                    None if logits_out is None else logits_out.data_ptr(),
                    None if choices_out is None else choices_out.data_ptr(),
                    logits_t0, None if self.context_tm is None else self.context_tm.data_ptr(),
                    self._sampling, _stream_ptr(self.device)), "mvn_generate_guided")
            return
        if self._per_seq is not None:
            with torch.cuda.device(self.device):
                N.check(self.lib.mvn_generate_seq(
                    self.dims, self.variant, self.packed.data_ptr(), self.state.data_ptr(),
                    self.samples.data_ptr(), self.batch, self.samples.stride(0), self.n_total, n_given,
                    t_begin, t_end, self._per_seq.data_ptr(),
                    None if logits_out is None else logits_out.data_ptr(),
                    None if choices_out is None else choices_out.data_ptr(),
                    logits_t0, None if self.context_tm is None else self.context_tm.data_ptr(),
                    self._sampling, _stream_ptr(self.device)), "mvn_generate_seq")
            return
        with torch.cuda.device(self.device):
            N.check(self.lib.mvn_generate_trunc(
                self.dims, self.variant, self.packed.data_ptr(), self.state.data_ptr(),
                self.samples.data_ptr(), self.batch, self.samples.stride(0), self.n_total, n_given,
                t_begin, t_end, self.temperature, self.seed,
                None if logits_out is None else logits_out.data_ptr(),
                None if choices_out is None else choices_out.data_ptr(),
                logits_t0, None if self.context_tm is None else self.context_tm.data_ptr(),
                self._sampling, self.top_k, self.top_p, _stream_ptr(self.device)), "mvn_generate_trunc")

    def _window(self, t_begin: int, n: int):
        """(buffer, ctx_t0, ctx_len) holding the context columns [t_begin, t_begin + n) of every row, written on the
        current stream.  A label alone: every column is the same, so the buffer is filled once (again only for a wider
        launch) and merely re-based."""
        from .ops import context_window
        src, C = self._source, self.dims.residual_channels
        if src.proj is None:
            if self._win is None or self._win_cols < n:
                self._win = context_window(None, 1, 0, n, glob=self.global_context)
                self._win_cols = n
            return self._win, t_begin, self._win_cols
        if self._win is None or self._win.numel() < self.nrows * n * C:
            self._win = torch.empty(self.nrows * n * C, dtype=torch.float32, device=self.device)
        context_window(src.proj, src.hop, t_begin, n, glob=self.global_context, proj_rows=self.batch, out=self._win)
        return self._win, t_begin, n

    def _run_windowed(self, t_begin: int, t_end: int, n_given: int, logits_out, choices_out, logits_t0: int) -> None:
        if t_end <= t_begin:
            return
        guided, scalar = self._guidance is not None, self._per_seq is None
        with torch.cuda.device(self.device):
            win, ctx_t0, ctx_len = self._window(t_begin, t_end - t_begin)
            N.check(self.lib.mvn_generate_windowed(
                self.dims, self.variant, self.packed.data_ptr(), self.state.data_ptr(),
                (self.samples_all if guided else self.samples).data_ptr(), self.batch, self.samples_all.stride(0),
                self.n_total, n_given, t_begin, t_end, self.temperature if scalar else 0.0, self.seed if scalar else 0,
                self.top_k if scalar else 0, self.top_p if scalar else 1.0,
                None if scalar else self._per_seq.data_ptr(), self._guidance.data_ptr() if guided else None,
                None if logits_out is None else logits_out.data_ptr(),
                None if choices_out is None else choices_out.data_ptr(), logits_t0, win.data_ptr(), ctx_t0, ctx_len,
                self._sampling, _stream_ptr(self.device)), "mvn_generate_windowed")

    def prime(self, prompt_idx: torch.Tensor) -> None:
        """Load a (B, P) prompt (P >= 1 class indices per sequence) and run the
        network over all but its last sample so that the queues are primed."""
        _require_gpu(prompt_idx, "prompt indices")
        B, P = prompt_idx.shape
        if B != self.batch or P < 1 or P > self.n_total:
            raise ValueError(f"prompt shape {tuple(prompt_idx.shape)} does not fit "
                             f"(batch {self.batch}, n_total {self.n_total})")
        self.reset()
        self.samples_all.zero_()
        self.samples[:, :P] = prompt_idx.to(torch.int32)
        if self._guidance is not None:  # the same prompt in both rows of a pair
            self.samples_all[:self.batch, :P] = self.samples[:, :P]
        self.n_given = P
        if self.prime_with_forward and P >= self.rf:
            # one full-sequence forward over the prompt (MFMA kernels), then copy
            # each layer's most recent d_l inputs into its queue
            from .ops import SequenceMode, run_forward
            idx = self.samples_all[:, :P].contiguous()
            ctx = None if self.context is None else self.context[:, :, :P]
            if self._source is not None and self._source.proj is not None:  # (all the frames: the clip's own edge clamp)
                ctx = self._source.prompt(P).detach().to(torch.float32)
                if self._guidance is not None:
                    ctx = torch.cat([ctx, ctx], 0)
            if self.global_context is not None:  # (the prompt's columns only: the steps read the time-major copy)
                g = self.global_context[:, :, None]
                ctx = g.expand(-1, -1, P) if ctx is None else ctx + g
            mode = SequenceMode(precision="fp16" if self.variant == N.GEN_PIPE_F16 else "fp32",
                                conditioning="none" if ctx is None else "context")
            _, buf = run_forward(self.dims, self._sd, idx, False, False, save=True, mode=mode, cond=ctx)
            with torch.cuda.device(self.device):
                N.check(self.lib.mvn_gen_prime_from_forward(
                    self.dims, buf.struct, self.nrows, P, self.state.data_ptr(),
                    _stream_ptr(self.device)), "mvn_gen_prime_from_forward")
        else:
            self._run(0, P - 1, P)
        self.t = P - 1

    def advance(self, n_new: int) -> None:
        """Generate n_new further samples per sequence."""
        t_end = min(self.t + n_new, self.n_total - 1)
        self._run(self.t, t_end, self.n_given)
        self.t = t_end

    def stream(self, n_new: int, chunk: int = 4000, deemphasis: float = 0.0, state=None):
        """Generate ``n_new`` further samples per sequence (after ``prime()``) and hand them out while they are being
        made: yields ``(t0, pcm)`` per launch of ``chunk`` steps (the last may be shorter) -- ``pcm`` the (batch, n)
        int16 numpy view of a pinned host buffer holding the 16-bit PCM (``mvn_pcm16_chunk``) of the columns
        [t0, t0 + n) just finished, valid until the next ``next()``.  Launch k + 1 is enqueued before the host waits
        for chunk k, so the GPU does not idle while the consumer handles a chunk.  A hand-off timeout of a pipelined
        variant raises ``PipeHandoffTimeout`` at the chunk where its status word is seen; ``check_errors()`` runs
        before the last chunk is handed out.  ``chunk < 1`` is a ValueError, raised here.

        ``deemphasis`` = a > 0 with ``state`` (``ops.pcm16_chunk``): the PCM of every chunk goes through the de-emphasis
        filter, whose (batch,) float64 state on the device -- zero, or as the prompt's columns left it -- is carried
        from chunk to chunk in ``state``."""
        chunks = plan_chunks(self.t + 1, min(int(n_new), self.n_total - 1 - self.t), chunk)
        return _stream_parts([(self, 0, self.batch)], self.batch, self.Q, chunks, self.device, self.check_errors,
                             deemphasis, state)

    def teacher_forced(self, indices: torch.Tensor, logits_t0: int):
        """Feed a fully given (B, n_total) history; return (choices, logits) for
        times >= logits_t0 -- used by the parity tests.  Guided: both rows of a pair are fed the history; the
        conditional rows' (choices, logits) are returned and ``teacher_forced_all`` keeps those of all 2 * batch rows."""
        if self._source is not None:
            raise RuntimeError("movenet_amd: teacher_forced runs on a whole-context generator (context= / "
                               "global_context=), not on one built with context_source")
        _require_gpu(indices, "indices")
        assert indices.shape == (self.batch, self.n_total)
        self.reset()
        self.samples.copy_(indices.to(torch.int32))
        if self._guidance is not None:
            self.samples_all[:self.batch].copy_(self.samples)
        logits = torch.zeros(self.nrows, self.n_total - logits_t0, self.Q, dtype=torch.float32,
                             device=self.device)
        choices = torch.full((self.nrows, self.n_total), -1, dtype=torch.int32, device=self.device)
        self._run(0, self.n_total - 1, self.n_total, logits, choices, logits_t0)
        self.t = self.n_total - 1
        self.teacher_forced_all = (choices, logits)
        return choices[self.nrows - self.batch:], logits[self.nrows - self.batch:]


# Measured cost model of a pipelined launch (DESIGN.md sections 4.1, 4.1c): its P pipelines serve
# ceil(n / P) sequences each in turn, and a step of ALL of them takes the pipeline's latency as long
# as the rounds fit under it, then rounds x the stages' service time per turn.  Keys: (C, variant);
# values: (us per step with one sequence per pipeline, us per step with several while the latency
# still bounds it, us per turn, most sequences per pipeline = GMAX of the kernel).
#   FOLD, config 2:  16 pipelines: 14.7 us for 16, 15.3 for 17 .. 80; beyond 80 sequences 23 pipelines (seven of
#                    them across XCDs: their slower hops set the latency): 16.4 us for 81 .. 128, 17.9 for 138,
#                    20.9 for 161, 23.2 for 184 (r2: 53 us for 64, 78 for 128)
#   PIPE, config 2:  24 pipelines: 17.4 us for 24 .. 96, 25.8 for 144, 34.4 for 192
#   PIPE, config 5:   4 pipelines: 72.4 us for 4, 73.2 for 5 .. 64 (the turn never bounds it)
_PIPELINED_US = {(64, N.GEN_FOLD): (14.7, 15.3, 2.64, 8), (64, N.GEN_PIPE): (17.4, 17.6, 4.3, 8),
                 (128, N.GEN_PIPE): (72.4, 73.2, 4.5, 16)}
_FOLD_CROSS_US = (16.4, 2.95)   # FOLD on all 23 pipelines: latency of a cross-XCD pipeline, us per turn
# ... and of the best kernel that takes EVERY sequence in one launch; keys: (C, conditioned):
# STREAM at C=64 without conditioning, GENERIC otherwise
# (r4: STREAM takes conditioning too -- (64, True) was GENERIC's 290 us)
_T_SINGLE_US = {(64, False): 78.0, (64, True): 100.0, (128, False): 490.0, (128, True): 490.0}

# The tables above were measured on ONE MI355X; boxes of a pool differ by up to 15 % and a cross-over between "k
# pipelined launches" and "one launch of the kernel that holds everything" moves with the RATIO of the two kernel
# families on the device at hand.  So the tables are only the SHAPE of the model: at first use per (device, C) the two
# families are timed once each on this device (`calibrate`) and the tables are scaled by measured / tabulated.
_CALIBRATION: dict = {}


def calibrate(dims, device=None, steps: int = 192) -> dict:
    """{"pipelined": measured / tabulated step time of one round of the pipelined kernel AUTO prefers, "single": the same
    for the one-launch kernel (STREAM or GENERIC)}, timed ONCE per (device, C, K, Q, L) with HIP events on synthetic weights
    (~0.1 s at config 2) and cached.  ``auto_plan`` multiplies its tables by these."""
    lib = N.lib()
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    key = (device.index, dims.layer_size, dims.stack_size, dims.input_channels, dims.residual_channels, dims.skip_channels)
    hit = _CALIBRATION.get(key)
    if hit is not None:
        return hit
    from .utils.weights import make_state_dict, synthetic_indices
    cfg = dict(layer_size=dims.layer_size, stack_size=dims.stack_size, input_channels=dims.input_channels,
               residual_channels=dims.residual_channels, skip_channels=dims.skip_channels)
    C = dims.residual_channels
    out = {"pipelined": 1.0, "single": 1.0}
    with torch.cuda.device(device):
        sd = {k: v.to(device) for k, v in make_state_dict(**cfg, seed=0).items()}
        rf = int(lib.mvn_receptive_fields(dims))
        one_launch = N.GEN_STREAM if lib.mvn_gen_variant(dims, N.GEN_STREAM, 1) == N.GEN_STREAM else N.GEN_GENERIC
        for kind, variant in (("pipelined", next((v for v in (N.GEN_FOLD, N.GEN_PIPE) if (C, v) in _PIPELINED_US and
                                                  lib.mvn_gen_variant(dims, v, 1) == v), None)),
                              ("single", one_launch)):
            if variant is None or (kind == "single" and (C, False) not in _T_SINGLE_US):
                continue
            n = max(1, lib.mvn_gen_launch_pipelines(dims, variant, 1 << 20)) if kind == "pipelined" else 4
            if kind == "pipelined":  # one round on the pipelines that sit inside one XCD (FOLD: 16 of the 23)
                n = max(1, lib.mvn_gen_launch_pipelines(dims, variant, min(n, 16)))
            g = RingGenerator(**cfg, state_dict=sd, batch=n, n_total=rf + 2 * steps + 2, device=device, variant=variant)
            g.prime(synthetic_indices(n, rf, dims.input_channels, 1234).to(device))
            g.advance(steps)  # warm-up (code objects, weights into place)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            g.advance(steps)
            ev[1].record()
            ev[1].synchronize()
            try:
                g.check_errors()
            except PipeHandoffTimeout:
                continue  # (a starved launch says nothing about the device: keep the table)
            us = ev[0].elapsed_time(ev[1]) * 1e3 / steps
            table = _PIPELINED_US[(C, variant)][0] if kind == "pipelined" else (
                _T_SINGLE_US[(C, False)] if variant == N.GEN_STREAM or C != 64 else 290.0)
            out[kind] = us / table
            out[kind + "_us_per_step"] = us
    _CALIBRATION[key] = out
    return out


def _launch_step_us(dims, variant: int, n: int):
    """Modelled step time (us) of ONE launch of ``variant`` holding ``n`` sequences, or None."""
    model = _PIPELINED_US.get((dims.residual_channels, variant))
    if model is None:
        return None
    t_one, t_multi, t_turn, gmax = model
    pipes = max(1, N.lib().mvn_gen_launch_pipelines(dims, variant, n))  # (FOLD: 16 up to 80 sequences, 23 beyond)
    rounds = -(-n // pipes)
    if variant == N.GEN_FOLD:
        lib = N.lib()
        every = lib.mvn_gen_launch_pipelines(dims, variant, 1 << 20)     # all the chip holds (config 2: 23)
        whole = lib.mvn_gen_launch_pipelines(dims, variant, 2 * every)   # those inside one XCD (16)
        if pipes > whole:                                                # the cross-XCD pipelines too
            t_multi, t_turn = _FOLD_CROSS_US
    return t_one if rounds <= 1 else max(t_multi, t_turn * rounds)


def auto_plan(dims, batch: int, has_context: bool, calibration=None, guided: bool = False):
    """``guided`` (classifier-free guidance: ``batch`` pairs): one launch of the best pipelined kernel
    whose pipelines hold the pairs (``mvn_gen_guided_max_pairs``; FOLD at config 2: 23), groups of at most that many
    pairs beyond it while the groups' modelled steps -- a launch's latency plus one turn -- add up to less than
    GENERIC's (the one-launch kernel with a guided form); not measured, the unguided tables stand in.
    ``calibration``: ``{"pipelined": f, "single": f}`` scale factors of the two kernel families on the device at hand
    (default: ``calibrate(dims)``, measured once at first need -- only batches beyond ONE pipelined launch consult it;
    pass ``{"pipelined": 1.0, "single": 1.0}`` for the tables as measured on the reference box).

    What MVN_GEN_AUTO means at the Python level for ``batch`` sequences: returns
    ``("single", 0, variant)`` for one launch or ``("grouped", group, variant)`` for groups of
    ``group`` sequences taking turns on the pipelines of a pipelined variant.

    Chosen on measured per-step cost (the table above).  C=K=64: ONE FOLD launch up to 184 sequences
    (16 pipelines up to 80 sequences, 23 beyond, x 8 rounds), then balanced groups of FOLD launches as long
    as they beat the one-launch kernels (STREAM 78 us / conditioned GENERIC ~0.3 ms for any number); the
    PIPE kernel's 24 pipelines are the fallback of the C library's AUTO for 185 .. 192.  C=K=128: ONE PIPE launch up to 64 sequences (4
    pipelines x 16 rounds, 73 us whatever the number), groups of up to 64 until GENERIC's 490 us is
    cheaper (beyond 384)."""
    lib = N.lib()
    C = dims.residual_channels
    if guided:
        for variant in (N.GEN_FOLD, N.GEN_PIPE):
            cap = max_pipe_batch(dims, variant, guided=True)
            model = _PIPELINED_US.get((C, variant))
            if cap <= 0 or model is None:
                continue
            k = -(-batch // cap)
            if k == 1:
                return "single", 0, variant
            # (placeholders, NOT measured: the unguided conditioned GENERIC step -- 290 us at C = 64 --, twice for the two
            # rows a guided workgroup runs, against a pipelined launch's latency plus one turn per group)
            generic_us = 290.0 if C == 64 else _T_SINGLE_US.get((C, True), 0.0)
            if k * (model[1] + model[2]) < 2 * generic_us:
                return "grouped", -(-batch // k), variant
            break
        return "single", 0, N.GEN_GENERIC
    single = N.check(lib.mvn_gen_variant(dims, N.GEN_AUTO, batch), "mvn_gen_variant")
    best = None
    for variant in (N.GEN_FOLD, N.GEN_PIPE):
        cap = max_pipe_batch(dims, variant)
        if cap <= 0 or (C, variant) not in _PIPELINED_US:
            continue
        k = -(-batch // cap)          # launches per step
        group = -(-batch // k)        # balanced: the step time of a launch grows with its rounds
        cost = k * _launch_step_us(dims, variant, group)
        if best is None or cost < best[0]:
            best = (cost, k, group, variant)
    if best is None:
        return "single", 0, single
    cost, k, group, variant = best
    if k == 1:
        return "single", 0, variant
    cal = calibration if calibration is not None else calibrate(dims)
    if cost * cal.get("pipelined", 1.0) < _T_SINGLE_US.get((C, bool(has_context)), 0.0) * cal.get("single", 1.0):
        return "grouped", group, variant
    return "single", 0, single  # the kernel the C library's AUTO names: every sequence in one launch


def max_pipe_batch(dims, variant: int = N.GEN_PIPE, guided: bool = False) -> int:
    """Largest batch one PIPE launch holds co-resident for these dims (0: no PIPE kernel); ``guided``: the most PAIRS
    of a guided launch (``mvn_gen_guided_max_pairs``: a pipeline per pair)."""
    lib = N.lib()
    if lib.mvn_gen_variant(dims, variant, 1) < 0:
        return 0
    if guided:
        return max(0, int(lib.mvn_gen_guided_max_pairs(dims, variant)))
    lo, hi = 1, 512
    while lo < hi:  # mvn_gen_variant is monotone in the batch
        mid = (lo + hi + 1) // 2
        if lib.mvn_gen_variant(dims, variant, mid) >= 0:
            lo = mid
        else:
            hi = mid - 1
    return lo


class GroupedGenerator:
    """More sequences than one pipelined launch can hold (FOLD: 184 at config 2, PIPE: 192;
    C = 128: 64): groups of sequences take turns on the pipelines, one launch per group per
    ``advance``; ``auto_plan`` picks this as long as the groups' step times add up to less than
    one launch of a kernel that holds every sequence (STREAM: 78 us).
    Same interface as ``RingGenerator``; ``samples`` is one (B, n_total) tensor the groups
    write their row blocks of.  Each group draws from its own Philox key (seed + group) -- unless any of
    ``temperature``, ``seed``, ``top_k``, ``top_p`` is a sequence of ``batch`` values (or ``rows`` is given): each group
    then receives its slice of the settings with the sequences' own seeds and their GLOBAL rows, and the samples are
    those of a single launch to the bit."""

    def __init__(self, layer_size, stack_size, input_channels, residual_channels, skip_channels,
                 state_dict, batch: int, n_total: int, device, group: int, temperature: float = 0.0,
                 seed: int = 0, context: Optional[torch.Tensor] = None, variant: int = N.GEN_PIPE,
                 sampling: str = "reference", top_k: int = 0, top_p: float = 1.0, rows=None,
                 global_context: Optional[torch.Tensor] = None, guidance=None,
                 context_source: Optional[ContextSource] = None):
        """``context_source``: as ``RingGenerator``'s; each group takes its own sequences' rows of it.
        ``guidance``: as ``RingGenerator``'s; the groups are then groups of ``group`` PAIRS, each sequence keeps
        its own settings and global row (as with per-sequence settings), and ``samples`` collects the groups'
        conditional rows after every ``prime`` / ``advance``."""
        N.sampling_rule(sampling)  # ValueError before anything is allocated
        self.sampling = sampling
        if context_source is not None and (context is not None or global_context is not None):
            raise ValueError("context_source replaces context and global_context: give one or the other")
        self.guidance = None if guidance is None else N.guidance_scales(batch, guidance)
        per_seq = None
        if self.guidance is not None or rows is not None or N.any_per_sequence(temperature, seed, top_k, top_p):
            host = N.seq_sampling_array(batch, input_channels, temperature, top_k, top_p, seed, rows)
            per_seq = [host[b] for b in range(int(batch))]
            self.top_k, self.top_p = [e.top_k for e in per_seq], [e.top_p for e in per_seq]
        else:
            self.top_k, self.top_p = N.truncation(top_k, top_p)  # (the same values for every group)
        self.batch, self.n_total, self.device = int(batch), int(n_total), torch.device(device)
        self.variant = variant
        self.samples = torch.zeros(self.batch, self.n_total, dtype=torch.int32, device=self.device)
        self.groups, self.bounds = [], []
        for gi, b0 in enumerate(range(0, self.batch, group)):
            b1 = min(self.batch, b0 + group)
            if per_seq is not None:
                mine = per_seq[b0:b1]
                settings = dict(temperature=[e.temperature for e in mine], seed=[e.seed for e in mine],
                                top_k=[e.top_k for e in mine], top_p=[e.top_p for e in mine],
                                rows=[e.row for e in mine])
            else:
                settings = dict(temperature=temperature, seed=(int(seed) + 0x9E3779B97F4A7C15 * gi) & (2 ** 64 - 1),
                                top_k=self.top_k, top_p=self.top_p)
            g = RingGenerator(layer_size, stack_size, input_channels, residual_channels, skip_channels,
                              state_dict, batch=b1 - b0, n_total=n_total, device=device,
                              variant=variant, context=None if context is None else context[b0:b1],
                              global_context=None if global_context is None else global_context[b0:b1],
                              sampling=sampling, guidance=None if self.guidance is None else self.guidance[b0:b1],
                              context_source=None if context_source is None else context_source.rows(b0, b1),
                              **settings)
            if self.guidance is None:
                g.samples = self.samples[b0:b1]  # a contiguous row block of the shared tensor
            self.groups.append(g)
            self.bounds.append((b0, b1))
        self.rf, self.dims = self.groups[0].rf, self.groups[0].dims

    def _collect(self) -> None:  # guided: a group's conditional rows are a view of ITS 2 x pairs rows
        if self.guidance is not None:
            for g, (b0, b1) in zip(self.groups, self.bounds):
                self.samples[b0:b1].copy_(g.samples)

    def prime(self, prompt_idx: torch.Tensor) -> None:
        for g, (b0, b1) in zip(self.groups, self.bounds):
            g.prime(prompt_idx[b0:b1])
        self._collect()

    def advance(self, n_new: int) -> None:
        for g in self.groups:
            g.advance(n_new)
        self._collect()

    def check_errors(self) -> None:
        for g in self.groups:
            g.check_errors()

    def stream(self, n_new: int, chunk: int = 4000, deemphasis: float = 0.0, state=None):
        """``RingGenerator.stream`` for the groups: per chunk one launch per group, each group's PCM into its row block
        of the chunk's buffer (through its row block of the de-emphasis ``state``), every group's status word beside it,
        one event behind them all."""
        t = self.groups[0].t
        chunks = plan_chunks(t + 1, min(int(n_new), self.n_total - 1 - t), chunk)

        def finish():
            self._collect()
            self.check_errors()
        parts = [(g, b0, b1) for g, (b0, b1) in zip(self.groups, self.bounds)]
        return _stream_parts(parts, self.batch, self.groups[0].Q, chunks, self.device, finish, deemphasis, state)


def plan_chunks(first: int, n_new: int, chunk: int):
    """The launches of a streamed generation: ``[(t0, n), ...]`` -- ``n_new`` columns from column ``first`` on in runs
    of ``chunk``, the last one shorter where ``chunk`` does not divide ``n_new``; none for ``n_new <= 0``.
    ``chunk < 1`` (or not an integer) is a ValueError."""
    if isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1:
        raise ValueError(f"chunk must be an integer >= 1, got {chunk!r}")
    first, n_new = int(first), max(int(n_new), 0)
    return [(first + k, min(chunk, n_new - k)) for k in range(0, n_new, chunk)]


def _stream_parts(parts, batch: int, classes: int, chunks, device, finish, deemphasis: float = 0.0, state=None):
    """What ``RingGenerator.stream`` and ``GroupedGenerator.stream`` share.  ``parts``: ``(generator, b0, b1)`` -- the
    generators that advance together and the rows of the chunk they own; ``finish``: run once everything has been
    enqueued and has completed, before the last chunk is handed out.  ``deemphasis`` > 0: the conversion is
    ``mvn_pcm16_deemph_chunk`` with the caller's (batch,) float64 ``state``, a part filtering through its own rows of it;
    a launch updates the state in stream order, so enqueueing ahead changes nothing.

    Per chunk, on the current stream: every part's launch, its ``mvn_pcm16_chunk`` into the device PCM buffer, one
    non-blocking copy of that buffer and one of every pipelined part's status word into the chunk's pinned host
    buffer (two of them, taking turns), and an event.  The host enqueues chunk k + 1, then waits for chunk k's event."""
    if deemphasis > 0.0 and (state is None or tuple(state.shape) != (batch,)):
        raise ValueError(f"deemphasis > 0 needs state: a ({batch},) float64 tensor on the device")
    if not chunks:
        finish()
        return
    import numpy as np
    from .ops import pcm16_chunk
    width = max(n for _, n in chunks)
    pcm_bytes = (2 * batch * width + 3) // 4 * 4  # the status words start on 4 bytes behind the PCM
    with torch.cuda.device(device):
        dev = torch.empty(batch * width, dtype=torch.int16, device=device)
        words = [g.status_word() for g, _, _ in parts]  # (None for a variant without hand-offs)
    host = [torch.zeros(pcm_bytes + 4 * len(parts), dtype=torch.uint8).pin_memory() for _ in range(2)]
    status = [h[pcm_bytes:].view(torch.int32) for h in host]
    status_np = [s.numpy() for s in status]

    def enqueue(k: int):
        t0, n = chunks[k]
        out = dev[:batch * n].view(batch, n)
        with torch.cuda.device(device):
            for g, b0, b1 in parts:
                g.advance(n)
                if deemphasis > 0.0:
                    pcm16_chunk(g.samples, t0, n, classes, out=out[b0:b1], deemphasis=deemphasis, state=state[b0:b1])
                else:
                    pcm16_chunk(g.samples, t0, n, classes, out=out[b0:b1])
            host[k % 2][:2 * batch * n].view(torch.int16).view(batch, n).copy_(out, non_blocking=True)
            for i, w in enumerate(words):
                if w is not None:
                    status[k % 2][i:i + 1].copy_(w, non_blocking=True)
            event = torch.cuda.Event()
            event.record(torch.cuda.current_stream(device))
        return event

    event = enqueue(0)
    for k, (t0, n) in enumerate(chunks):
        ahead = enqueue(k + 1) if k + 1 < len(chunks) else None
        wait_event(event)
        if np.any(status_np[k % 2] != 0):
            raise PipeHandoffTimeout(
                "movenet_amd: PIPE generator hand-off timed out (pipeline stages not co-resident); the samples from "
                f"column {t0} on are not valid")
        if ahead is None:
            finish()
        yield t0, host[k % 2][:2 * batch * n].view(torch.int16).view(batch, n).numpy()
        event = ahead
