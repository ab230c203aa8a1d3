"""AdamW / Adam over ONE flat parameter buffer: one HIP kernel per optimizer step
(``mvn_adamw_step``) instead of torch's per-tensor / foreach kernels (row F3 of SURVEY.md
section 8; the optimizer the reference's ``configure_optimizers`` builds,
/root/reference/movenet/pytorch_lightning_trainer.py:186-189).

The parameters keep their identity (``nn.Parameter`` objects, ``state_dict`` names) but their
storage is re-pointed into one flat fp32 buffer, in the order the decoder's backward lays its
gradients out (``ops.decoder_param_names``).  ``ops._run_backward`` returns the gradients as
views of one flat buffer in the same order, so a step is ONE launch over
(parameters, gradients, exp_avg, exp_avg_sq); parameters without a gradient (the last layer's
residual conv, unused video / context parameters) are skip ranges of that launch, exactly as
torch leaves them alone.  Gradients that do not lie in one buffer (the eight video-encoder
tensors, or a caller's own) are stepped with one launch of the same kernel per tensor.

``ema_decay > 0`` keeps an exponential moving average of the parameters in a second flat buffer (``self.ema``),
updated by the same launches (``mvn_adamw_ema_step``: the step's kernel with one more read-modify-write).
``averaged_parameters()`` re-points the parameters into that buffer and back -- no copy either way -- so validation and
sampling run on the averaged weights; ``ema_state_dict(model)`` is what a checkpoint saves of them.

A ``torch.optim.Optimizer`` subclass: ``param_groups`` (so the torch LR schedulers drive
``lr``), ``zero_grad`` and ``state_dict`` behave as usual; one parameter group.
"""
from __future__ import annotations

import contextlib
import ctypes
from typing import Iterable, List, Optional, Tuple

import torch

from . import _native as N


def ema_decay_at(decay: float, t: int, warmup: bool) -> float:
    """The decay of the average's update ``t`` (0 for the first): ``decay``, or with ``warmup``
    ``min(decay, (1 + t) / (10 + t))`` -- 0.1, 2/11, ... -- so that the early average follows the parameters
    instead of remembering their initial values for 1 / (1 - decay) steps."""
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


class FlatAdamW(torch.optim.Optimizer):
    def __init__(self, params: Iterable[torch.nn.Parameter], lr: float = 1e-3,
                 betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, decoupled: bool = True, ema_decay: float = 0.0,
                 ema_warmup: bool = True):
        params = [p for p in params]
        if not 0.0 <= ema_decay < 1.0:  # (NaN fails both comparisons)
            raise ValueError(f"FlatAdamW: ema_decay must lie in [0, 1), got {ema_decay!r}")
        if not params:
            raise ValueError("FlatAdamW: no parameters")
        dev = params[0].device
        if dev.type != "cuda":
            raise RuntimeError("movenet_amd.FlatAdamW steps on an MI355X device; no CPU path exists")
        for p in params:
            if p.device != dev or p.dtype != torch.float32:
                raise ValueError("FlatAdamW: all parameters must be fp32 on one device")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                      decoupled=decoupled))
        self._params: List[torch.nn.Parameter] = params
        self._offsets: List[int] = []
        off = 0
        for p in params:
            self._offsets.append(off)
            off += p.numel()
        self._n = off
        with torch.no_grad():
            self.flat = torch.empty(off, dtype=torch.float32, device=dev)
            for p, o in zip(params, self._offsets):
                self.flat[o:o + p.numel()].copy_(p.detach().reshape(-1))
                p.data = self.flat[o:o + p.numel()].view(p.shape)  # same values, flat storage
        self.exp_avg = torch.zeros_like(self.flat)
        self.exp_avg_sq = torch.zeros_like(self.flat)
        # torch counts steps PER PARAMETER (one that first receives a gradient at step 4 is
        # bias-corrected as step 1): kept here on the host, a run of parameters shares one count
        self._steps: List[int] = [0] * len(params)
        self.ema_decay, self.ema_warmup = float(ema_decay), bool(ema_warmup)
        self.ema_updates = 0      # calls of step() so far: the t of ema_decay_at
        self._averaged = False    # inside averaged_parameters()
        if self.ema_decay > 0:
            self.ema = self.flat.clone()  # (after the copy above: the average starts at the parameters)
        self._point_state()
        self.last_launches = 0

    def _point_state(self) -> None:
        flat = {"steps": self._steps, "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq}
        if self.ema_decay > 0:
            flat.update(ema=self.ema, ema_updates=self.ema_updates)
        self.state["flat"] = flat

    # ------------------------------------------------------------------
    def load_state_dict(self, state_dict) -> None:
        """torch's ``Optimizer.load_state_dict`` REPLACES ``self.state`` with new objects; the
        moments this optimizer steps over are the flat buffers made in the constructor, so the
        loaded moments and per-parameter step counts are copied INTO them (and ``self.state``
        is pointed back at them): a resumed run continues where the saved one stopped."""
        flat = state_dict["state"].get("flat") if "state" in state_dict else None
        if flat is None:
            raise ValueError("FlatAdamW.load_state_dict: no 'flat' entry (not a FlatAdamW state_dict)")
        steps, m, v = list(flat["steps"]), flat["exp_avg"], flat["exp_avg_sq"]
        if len(steps) != len(self._params) or m.numel() != self._n or v.numel() != self._n:
            raise ValueError(f"FlatAdamW.load_state_dict: saved state covers {len(steps)} parameters / "
                             f"{m.numel()} elements, this optimizer {len(self._params)} / {self._n}")
        super().load_state_dict(state_dict)  # param_groups (lr, betas, ...) as torch does it
        with torch.no_grad():
            self.exp_avg.copy_(m.reshape(-1))
            self.exp_avg_sq.copy_(v.reshape(-1))
            if self.ema_decay > 0:
                # (a state saved without the average: it starts over from the current parameters)
                saved = flat.get("ema")
                if saved is not None and saved.numel() != self._n:
                    raise ValueError(f"FlatAdamW.load_state_dict: saved average covers {saved.numel()} elements, "
                                     f"this optimizer {self._n}")
                self.ema.copy_(self.flat if saved is None else saved.reshape(-1))
                self.ema_updates = 0 if saved is None else int(flat.get("ema_updates", 0))
        self._steps[:] = [int(x) for x in steps]
        self._point_state()

    # ------------------------------------------------------------------
    @contextlib.contextmanager
    def averaged_parameters(self):
        """Inside, every parameter's ``.data`` is its view of ``self.ema``; on exit (also by an exception) the views
        into ``self.flat`` are back.  Nothing is copied.  RuntimeError when nested, with the average off, and for a
        ``step()`` inside."""
        if self.ema_decay <= 0:
            raise RuntimeError("FlatAdamW.averaged_parameters: the average is off (ema_decay = 0)")
        if self._averaged:
            raise RuntimeError("FlatAdamW.averaged_parameters: already inside (not re-entrant)")
        self._averaged = True
        self._repoint(self.ema)
        try:
            yield self
        finally:
            self._repoint(self.flat)
            self._averaged = False

    @property
    def inside_average(self) -> bool:
        """True inside ``averaged_parameters()``: the parameters point into ``self.ema``."""
        return self._averaged

    def _repoint(self, buf: torch.Tensor) -> None:
        for p, o in zip(self._params, self._offsets):
            p.data = buf[o:o + p.numel()].view(p.shape)

    def ema_state_dict(self, model: torch.nn.Module):
        """``model.state_dict()`` with every optimized parameter replaced by its average (detached clones); buffers
        and parameters outside this optimizer as they are."""
        if self.ema_decay <= 0:
            raise RuntimeError("FlatAdamW.ema_state_dict: the average is off (ema_decay = 0)")
        where = {id(p): i for i, p in enumerate(self._params)}
        names = {n: where[id(p)] for n, p in model.named_parameters() if id(p) in where}
        out = model.state_dict()
        for n, i in names.items():
            o = self._offsets[i]
            out[n] = self.ema[o:o + self._params[i].numel()].view(self._params[i].shape).detach().clone()
        return out

    def _launch(self, p_ptr, g_ptr, m_ptr, v_ptr, n, step, skips, stream, e_ptr=None, ema_w=0.0) -> None:
        grp = self.param_groups[0]
        arr = (ctypes.c_size_t * max(2 * len(skips), 1))(*[x for r in skips for x in r])
        if e_ptr is not None:
            N.check(N.lib().mvn_adamw_ema_step(p_ptr, g_ptr, m_ptr, v_ptr, e_ptr, n, float(grp["lr"]),
                                               float(grp["betas"][0]), float(grp["betas"][1]), float(grp["eps"]),
                                               float(grp["weight_decay"]), step, int(bool(grp["decoupled"])),
                                               ema_w, arr, len(skips), stream), "mvn_adamw_ema_step")
            self.last_launches += 1
            return
        N.check(N.lib().mvn_adamw_step(p_ptr, g_ptr, m_ptr, v_ptr, n, float(grp["lr"]),
                                       float(grp["betas"][0]), float(grp["betas"][1]), float(grp["eps"]),
                                       float(grp["weight_decay"]), step, int(bool(grp["decoupled"])),
                                       arr, len(skips), stream), "mvn_adamw_step")
        self.last_launches += 1

    def _spans(self):
        """Greedy partition of the parameters (in flat order) into runs whose gradients mirror
        the flat parameter layout inside ONE gradient storage: (first, last_exclusive, skips)."""
        runs, i, P = [], 0, self._params
        while i < len(P):
            g = P[i].grad
            if g is None:
                i += 1
                continue
            ok = g.dtype == torch.float32 and g.is_contiguous() and g.device == self.flat.device
            if not ok:
                raise ValueError("FlatAdamW: gradients must be contiguous fp32 on the parameters' device")
            store, base = g.untyped_storage().data_ptr(), g.storage_offset() - self._offsets[i]
            j, skips, pending = i + 1, [], None
            last = i + 1
            while j < len(P):
                gj = P[j].grad
                if gj is None:
                    if pending is None:
                        pending = j
                    j += 1
                    continue
                same = (gj.dtype == torch.float32 and gj.is_contiguous()
                        and gj.untyped_storage().data_ptr() == store
                        and gj.storage_offset() - self._offsets[j] == base
                        and self._steps[j] == self._steps[i])
                if not same:
                    break
                if pending is not None:
                    if len(skips) == 4:
                        break
                    skips.append((self._offsets[pending] - self._offsets[i],
                                  self._offsets[j] - self._offsets[i]))
                    pending = None
                j += 1
                last = j
            runs.append((i, last, skips))
            i = last
        return runs

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._averaged:
            raise RuntimeError("FlatAdamW.step inside averaged_parameters(): the parameters point into the average")
        dev = self.flat.device
        self.last_launches = 0
        on = self.ema_decay > 0
        # 1 - decay in double, rounded once to the float the kernel multiplies by
        ema_w = 1.0 - ema_decay_at(self.ema_decay, self.ema_updates, self.ema_warmup) if on else 0.0
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            for first, last, skips in self._spans():
                step = self._steps[first] + 1
                for k in range(first, last):
                    if self._params[k].grad is not None:
                        self._steps[k] = step
                o0 = self._offsets[first]
                end = self._offsets[last - 1] + self._params[last - 1].numel()
                g0 = self._params[first].grad
                self._launch(self.flat.data_ptr() + 4 * o0, g0.data_ptr(), self.exp_avg.data_ptr() + 4 * o0,
                             self.exp_avg_sq.data_ptr() + 4 * o0, end - o0, step, skips, stream,
                             self.ema.data_ptr() + 4 * o0 if on else None, ema_w)
        if on:
            self.ema_updates += 1
            self.state["flat"]["ema_updates"] = self.ema_updates
        return loss


def order_like_backward(model, with_context: bool = False) -> List[torch.nn.Parameter]:
    """The model's parameters in the order ops._run_backward lays their gradients out for an
    audio-only (``with_context=False``) or a video-conditioned run, then everything else
    (context convs of an audio-only run, video encoder).  With the matching order a step is
    one launch (plus one per video tensor); with the other order it is still correct, in
    more launches."""
    from .ops import decoder_param_names
    lookup = dict(model.named_parameters())
    L = model.layer_size * model.stack_size
    names = decoder_param_names(L, with_context=with_context)
    seen = set(names)
    ordered = [lookup[n] for n in names] + [p for n, p in lookup.items() if n not in seen]
    return [p for p in ordered if p.requires_grad]
