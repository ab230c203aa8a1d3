"""GPU: mvn_forward / mvn_backward and their _f16 / _bf16 siblings through ctypes, on poisoned buffers, against float64.

Every other test reaches these entry points through movenet_amd/ops.py, the friendliest possible caller: gradients
into zeros, scratch out of the allocator's recycled (finite) memory, tight strides, only logits and parameter gradients
compared.  Here the four entry points are called directly (N.lib(), N.FwdBuffers / BwdBuffers / ParamGrads,
ops.pack_params) and every buffer of a call is carved out of a larger allocation with a sentinel band behind it AND in
front of it (helpers._Guard), filled in its whole extent before the call:

  acts, th, sg, z, skip, a1, out and the seven backward buffers ......... NaN
  dlogit on the dout == NULL path ........ NaN, then written by mvn_softmax_ce_backward with ops.py's arguments
  index columns >= t_len (index_stride > t_len) .......................... 0x7fffffff and -1, alternating
  ctx columns >= t_len (ctx_ld = Tp or wider), dense_audio columns >= t_len ..... NaN
  every gradient tensor ..... a seeded g0 at the scale of the float64 gradient's largest entry (the library
                              ACCUMULATES: what is compared is grad - g0, one fp32 ulp of that scale worse at most)

The reference is oracle.wavenet_oracle in float64 with torch autograd (causal_conv, gated_layer, dense_head; tanh(f)
and sigmoid(g), which gated_layer does not return, restated from its first lines).  Bounds, none derived from the
code under test: forward values 2e-5 of the tensor's own largest entry (LOGIT_TOL); gradients helpers.grad_bound(dev),
dev = the deviation of the same oracle run in float32 on the CPU; bf16 entry points against tests/bf16_emulation.py
with test_bf16_train_gpu.py's own criteria (_check_grads, logits error <= 2 x the emulation's); mvn_forward_f16
5e-3 of the logit range (FP16_TOL of test_fp16_forward_mfma_within_tolerance).

After a call: both bands of every buffer intact; out written in full and finite; the valid region of every saved
tensor finite and within bound (acts[l]: A_l <= t < T for l < L -- plane L is never written, the header now says so,
and must still hold its fill; th[l], sg[l]: A_{l+1} <= t < T; skip, a1: columns pad .. pad + S; dctx[:, :, :T], and
dctx's columns >= T zero: the header now promises "written in full"); grad - g0 within bound, and BIT-EQUAL to g0 for
the last layer's residual conv and, without a context, the ctx_* tensors; index, ctx, dense_audio, the parameters, out
and dout bit-identical after mvn_backward; a SECOND mvn_backward over the same saved forward, re-poisoned scratch and
fresh g0, within the same bounds, with every saved tensor but z bit-identical before the first and after the second
(z is shared scratch of the two passes: the header now says so).

Branches (C = K = 64, Q = 256; constants from the sources, asserted per row by _branches):
  FS3_PACK_F = 36992, FSC_PACK_F = 40960 floats (fused_fwd_bf3.h:108,147,364), DS3_IMG_F = 123392, DS3_BWD_IMG_F =
  123200 (fused_fwd_bf3.h:837-839); g.act = B 64 Tp.
  z "layers":   g.act >= L FS3_PACK_F                                   (sequence.hip forward_impl, `bf3 && ...`)
  z "fwd head": g.act >= L FSC_PACK_F + DS3_IMG_F                       (forward_impl, `head_img`)
  z "bwd head": g.act >= L FSC_PACK_F + DS3_IMG_F + DS3_BWD_IMG_F       (plan_backward, `BwdPlan::head_img`)
  bias "reserved": max(ceil((T + 31) / 512) B, 2 CUs + B) 128 <= B Q Sp / 2   (plan_backward, `BwdPlan::bias2`)
  bias "small":    not reserved and  B Q Sp / 24704 >= B                       (plan_backward, `BwdPlan::sc_bias`)
  bias "none":     neither: no one-kernel form, mvn_last_backward_form() == 1
  head_scratch_ok: ceil((S + 31) / 512) B 256 257 <= B 128 Tp                  (plan_backward, `BwdPlan::head_bias`)

Largest errors seen on an MI355X (256 CUs; the file runs in 17 s), printed per case with pytest -s:
  forward, fp32 entry point (bound 2e-5) ... out 4.7e-7, acts 4.2e-7, th 7.8e-7, sg 2.3e-7, skip 2.8e-7, a1 2.3e-7
  parameter gradients ....................... 9.3e-6 against grad_bound 2.7e-5 (layer 4 gate weight; 10 x 3, B 5, T 4700)
  dctx ...................................... 7.5e-7 against 2e-5
  bf16 ...................................... logits 2.4e-3 (emulation 2.0e-3 .. 2.3e-3), worst cosine 0.99817 (0.99869)
Nothing failed under the poison: the only defects were host-side argument handling (mvn_forward checked the context
arguments behind its first launch; mvn_backward did not check index_stride / dense_ld / ctx_ld at all, and refused
out = NULL with dout given when S_out = 0).  Mutations of a scratch copy, one run each: `*dst = t` for `*dst += t` in
slab_reduce_kernel failed 57 of the 77 cases (pre-filled gradients); the th edge load of bwd_layer64_kernel masked one
tile later (min(te + 64, Tp): in bounds) failed 29 (NaN in the filter / gate weight gradients).
"""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

import bf16_emulation as E
from helpers import DEV, _Guard, grad_bound
from movenet_amd import _native as N
from movenet_amd import ops
from movenet_amd.utils.weights import make_state_dict, synthetic_indices
from oracle import wavenet_oracle as O

pytestmark = pytest.mark.gpu
NAN = float("nan")
LOGIT_TOL = 2e-5
FP16_TOL = 5e-3
FS3_PACK_F, FSC_PACK_F, DS3_IMG_F, DS3_BWD_IMG_F, FB16_PACK_F = 36992, 40960, 123392, 123200, 12416
SWITCHES = ("MOVENET_HIP_NO_FUSED_FORWARD", "MOVENET_HIP_FORWARD_MFMA", "MOVENET_HIP_FORWARD_TILE",
            "MOVENET_HIP_BWD_FORM", "MOVENET_HIP_NO_FUSED_BACKWARD")
ENTRY = {"f32": ("mvn_forward", "mvn_backward"), "bf16": ("mvn_forward_bf16", "mvn_backward_bf16"),
         "f16": ("mvn_forward_f16", None)}


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _err(got, want):
    return ((got.double().cpu() - want.double()).abs().max() / want.double().abs().max().clamp_min(1e-30)).item()


def _bits(t):
    return t.detach().reshape(-1).view(torch.int32).clone()


def _ptr(t):
    return None if t is None else t.data_ptr()


class Case:
    """One call: dims, batch, length, flags and strides.  ctx: None | "tight" (ctx_ld = Tp) | "wide"."""

    def __init__(self, ls, ss, Q, C, K, B, T, ctx=None, dense=False, wide=False, norm=False, rl=False, dout=True):
        self.ls, self.ss, self.Q, self.C, self.K, self.B, self.T = ls, ss, Q, C, K, B, T
        self.ctx, self.dense, self.wide, self.norm, self.rl, self.dout = ctx, dense, wide, norm, rl, dout
        self.dims = O.Dims(ls, ss, Q, C, K)
        self.L, self.RF = self.dims.n_layers, self.dims.receptive_fields
        self.S = T - self.RF + 1
        self.S_out = self.S - (1 if rl else 0)
        self.A = [0]
        for d in self.dims.dilations:
            self.A.append(self.A[-1] + d)
        self.pad = (self.RF - 1) & 31

    def key(self):
        return (self.ls, self.ss, self.Q, self.C, self.K, self.B, self.T, self.ctx is not None, self.dense, self.norm,
                self.rl, self.dout)

    def __repr__(self):
        s = f"{self.ls}x{self.ss} Q{self.Q} C{self.C} K{self.K} B{self.B} T{self.T}"
        for flag in ("ctx", "dense", "wide", "norm", "rl"):
            if getattr(self, flag):
                s += f" {flag}={getattr(self, flag)}" if flag == "ctx" else f" {flag}"
        return s + ("" if self.dout else " dout=NULL")


# ---- data and the float64 reference -------------------------------------------------------------------------------
def _key(l, name):
    return f"residual_conv_stack.conv_layers.{l}.{name}"


def _oracle(c, sd, x, ctx, up, target, dtype, logits_fn=None):
    """The forward of wavenet_oracle.logits_full with every per-layer value kept, and autograd's gradients"""
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items() if not k.startswith("video")}
    cx = None if ctx is None else ctx.to(dtype).clone().requires_grad_(True)
    r = dict(acts=[], th=[], sg=[])
    if logits_fn is not None:   # (the bf16 emulation: logits and gradients only)
        logits = logits_fn(p, c.dims, x.to(dtype))
    else:
        h = O.causal_conv(p, x.to(dtype))
        skips = []
        for l, d in enumerate(c.dims.dilations):
            r["acts"].append(h.detach())
            f = F.conv1d(h, p[_key(l, "conv_filter.conv.weight")], dilation=d)   # modules.py:67-79, as gated_layer
            g = F.conv1d(h, p[_key(l, "conv_gate.conv.weight")], dilation=d)
            if cx is not None:
                cc = cx[:, :, -f.size(2):]
                f = f + F.conv1d(cc, p[_key(l, "context_conv_filter.weight")], p[_key(l, "context_conv_filter.bias")])
                g = g + F.conv1d(cc, p[_key(l, "context_conv_gate.weight")], p[_key(l, "context_conv_gate.bias")])
            r["th"].append(torch.tanh(f).detach())
            r["sg"].append(torch.sigmoid(g).detach())
            h, s = O.gated_layer(p, l, d, h, cx, c.S)
            skips.append(s)
        skip = torch.sum(torch.stack(skips), dim=0)
        r["skip"] = skip.detach()
        r["a1"] = F.leaky_relu(F.conv1d(F.leaky_relu(skip), p["dense_conv.conv1.weight"],
                                        p["dense_conv.conv1.bias"])).detach()
        logits = O.dense_head(p, skip)
    out = logits[:, :, :-1] if c.rl else logits
    if c.norm:
        out = F.softmax(out, dim=1)
    r["out"] = out.detach()
    if c.S_out > 0:
        # dout == NULL: the trainer's loss, cross_entropy on PROBABILITIES (pytorch_lightning_trainer.py:64-66)
        loss = (out * up.to(dtype)).sum() if c.dout else F.cross_entropy(out, target)
        loss.backward()
    r["grads"] = {k: v.grad for k, v in p.items()}
    r["dctx"] = None if cx is None else cx.grad
    return r


@functools.lru_cache(maxsize=None)
def _data(key):
    """Seeded inputs of a case and its float64 reference (once per module), the same oracle in float32, and g0"""
    c = Case(*key[:7], ctx="tight" if key[7] else None, dense=key[8], norm=key[9], rl=key[10], dout=key[11])
    seed = sum(int(v) * w for v, w in zip(key, (7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47)))
    sd = make_state_dict(c.ls, c.ss, c.Q, c.C, c.K, seed=seed)
    gen = torch.Generator().manual_seed(seed)
    idx = synthetic_indices(c.B, c.T, c.Q, seed + 1)
    if c.dense:   # not one-hot: a dense (B, Q, T) input at the scale of a one-hot column
        x = torch.randn(c.B, c.Q, c.T, generator=gen) / c.Q ** 0.5
    else:
        x = F.one_hot(idx, c.Q).permute(0, 2, 1).to(torch.float32)
    ctx = torch.randn(c.B, c.C, c.T, generator=gen) if key[7] else None
    up = torch.randn(c.B, c.Q, max(c.S_out, 0), generator=gen)
    target = torch.randint(0, c.Q, (c.B, max(c.S_out, 0)), generator=gen)
    ref = _oracle(c, sd, x, ctx, up, target, torch.float64)
    ref32 = _oracle(c, sd, x, ctx, up, target, torch.float32)
    dev, g0 = {}, {}
    for k, g in ref["grads"].items():
        dev[k] = 0.0 if g is None else _err(ref32["grads"][k], g)
        scale = 1.0 if g is None or float(g.abs().max()) == 0.0 else float(g.abs().max())
        g0[k] = (torch.randn(sd[k].shape, generator=gen) * scale).to(torch.float32)
    dev["dctx"] = 0.0 if ctx is None or ref["dctx"] is None else _err(ref32["dctx"], ref["dctx"])
    return dict(sd=sd, idx=idx, x=x, ctx=ctx, up=up, target=target, ref=ref, dev=dev, g0=g0)


def _wide(n):
    """a leading dimension above n: the next multiple of 64 past it, plus 64"""
    return (n + 64) // 64 * 64 + 64


# ---- one call of the library on poisoned buffers -------------------------------------------------------------------
class Run:
    def __init__(self, c, entry="f32", save=True):
        lib = N.lib()
        self.c, self.entry, self.save, self.g = c, entry, save, _Guard(front=True)
        self.d = _data(c.key())
        self.dims = N.make_dims(c.ls, c.ss, c.Q, c.C, c.K)
        assert lib.mvn_receptive_fields(self.dims) == c.RF
        self.Tp, self.Sp = lib.mvn_padded_len(c.T), lib.mvn_padded_len(c.S + 31)
        new, B, C, K, Q, L, T = self.g.new, c.B, c.C, c.K, c.Q, c.L, c.T
        self.pd = {k: self.g.put(v, k) for k, v in self.d["sd"].items() if not k.startswith("video")}
        self.params, self._keep = ops.pack_params(self.dims, self.pd, L)
        self.inputs = dict(self.pd)
        self.index = self.dense = self.ctx = None
        self.istride = self.dense_ld = self.ctx_ld = 0
        if c.dense:
            self.dense_ld = _wide(T)   # (always wide: ops.py only ever passes dense_ld == t_len)
            self.dense = new((B, Q, self.dense_ld), NAN, "dense_audio")
            self.dense[:, :, :T] = self.d["x"].to(DEV)
            self.inputs["dense_audio"] = self.dense
        else:
            self.istride = _wide(T) if c.wide else T
            self.index = new((B, self.istride), None, "index", dtype=torch.int32)
            self.index[:, 0::2] = 0x7fffffff
            self.index[:, 1::2] = -1
            self.index[:, :T] = self.d["idx"].to(DEV, torch.int32)
            self.inputs["index"] = self.index
        if c.ctx:
            self.ctx_ld = self.Tp if c.ctx == "tight" else _wide(self.Tp)
            self.ctx = new((B, C, self.ctx_ld), NAN, "ctx")
            self.ctx[:, :, :T] = self.d["ctx"].to(DEV)
            self.inputs["ctx"] = self.ctx
        n_act = L + 1 if save else 2
        self.fwd = dict(acts=new((n_act, B, C, self.Tp), NAN, "acts"), z=new((B, C, self.Tp), NAN, "z"),
                        skip=new((B, K, self.Sp), NAN, "skip"), a1=new((B, Q, self.Sp), NAN, "a1"))
        if save:
            self.fwd.update(th=new((L, B, C, self.Tp), NAN, "th"), sg=new((L, B, C, self.Tp), NAN, "sg"))
        self.out = new((B, Q, max(c.S_out, 0)), NAN, "out")
        f = self.fwd
        self.fb = N.FwdBuffers(_ptr(f["acts"]), _ptr(f.get("th")), _ptr(f.get("sg")), _ptr(f["z"]), _ptr(f["skip"]),
                               _ptr(f["a1"]), _ptr(self.ctx), self.ctx_ld, _ptr(self.dense), self.dense_ld)
        self.bwd = self.grads = self.dout = None

    # -- forward
    def forward(self, **over):
        c = self.c
        a = dict(dims=self.dims, params=self.params, index=_ptr(self.index), istride=self.istride, B=c.B, T=c.T, fb=self.fb,
                 out=_ptr(self.out) if c.S_out > 0 else None, norm=int(c.norm), rl=int(c.rl), save=int(self.save))
        a.update(over)
        return getattr(N.lib(), ENTRY[self.entry][0])(a["dims"], a["params"], a["index"], a["istride"], a["B"], a["T"],
                                                      a["fb"], a["out"], a["norm"], a["rl"], a["save"], _stream())

    def check_forward(self, what, tol=LOGIT_TOL, values=True):
        c, ref = self.c, self.d["ref"]
        self.g.check(f"{what}: forward")
        worst = {}

        def close(name, got, want):
            assert bool(torch.isfinite(got).all()), (c, what, name, "not finite")
            e = _err(got, want)
            cls = name.split("[")[0]
            worst[cls] = max(worst.get(cls, 0.0), e)
            assert e < tol, (c, what, name, e, tol)

        if c.S_out > 0:   # written in full; what lies past S_out is the band behind it
            close("out", self.out, ref["out"])
        if self.save:
            for name in ("acts", "th", "sg", "skip", "a1"):
                assert bool(torch.isfinite(self.valid(name)[0]).all()), (c, what, name, "not finite")
            # plane L of acts, the last layer's residual output, is never produced: the caller's NaN is still there
            assert bool(torch.isnan(self.fwd["acts"][c.L]).all()), (c, what, "acts[L] was written")
        if self.save and values:
            for l in range(c.L):
                close(f"acts[{l}]", self.fwd["acts"][l][:, :, c.A[l]:c.T], ref["acts"][l])
                close(f"th[{l}]", self.fwd["th"][l][:, :, c.A[l + 1]:c.T], ref["th"][l])
                close(f"sg[{l}]", self.fwd["sg"][l][:, :, c.A[l + 1]:c.T], ref["sg"][l])
            close("skip", self.fwd["skip"][:, :, c.pad:c.pad + c.S], ref["skip"])
            close("a1", self.fwd["a1"][:, :, c.pad:c.pad + c.S], ref["a1"])
        print(f"forward  {c} [{what}]: " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()) + f" / {tol:.0e}")
        return worst

    def valid(self, name):
        """the documented valid regions of a saved tensor, as a list of views"""
        c, t = self.c, self.fwd[name]
        if name == "acts":
            return [torch.cat([t[l][:, :, c.A[l]:c.T].reshape(-1) for l in range(c.L)])]
        if name in ("th", "sg"):
            return [torch.cat([t[l][:, :, c.A[l + 1]:c.T].reshape(-1) for l in range(c.L)])]
        return [t[:, :, c.pad:c.pad + c.S]]

    # -- backward
    def grad_struct(self, without=()):
        gp, self._gkeep = ops.pack_params(self.dims, {k: v for k, v in self.grads.items()}, self.c.L)
        g = N.ParamGrads(gp.causal_w, gp.filter_w, gp.gate_w, gp.residual_w, gp.residual_b, gp.skip_w, gp.skip_b,
                         gp.head1_w, gp.head1_b, gp.head2_w, gp.head2_b, gp.ctx_filter_w, gp.ctx_filter_b,
                         gp.ctx_gate_w, gp.ctx_gate_b)
        for name in without:
            setattr(g, name, None)
        return g

    def prepare_backward(self):
        """(re-)poisons the seven scratch buffers, (re-)fills the gradients with g0, writes dout / dlogit"""
        c, new, B, C, K, Q = self.c, self.g.new, self.c.B, self.c.C, self.c.K, self.c.Q
        if self.bwd is None:
            self.bwd = dict(dx_a=new((B, C, self.Tp), None, "dx_a"), dx_b=new((B, C, self.Tp), None, "dx_b"),
                            dfg=new((B, 2 * C, self.Tp), None, "dfg"), dskip=new((B, K, self.Sp), None, "dskip"),
                            da1=new((B, Q, self.Sp), None, "da1"), dlogit=new((B, Q, self.Sp), None, "dlogit"))
            if c.ctx:
                self.bwd["dctx"] = new((B, C, self.Tp), None, "dctx")
            self.grads = {k: new(tuple(v.shape), None, "grad " + k) for k, v in self.d["g0"].items()}
            self.dout = self.g.put(self.d["up"].to(DEV), "dout") if c.dout else None
        for t in self.bwd.values():
            t.fill_(NAN)
        for k, t in self.grads.items():
            t.copy_(self.d["g0"][k])
        if not c.dout and c.S_out > 0:
            # ops.py (_WaveNetLossFunction.backward): the loss differentiated straight into dlogit, S + 1 columns
            assert c.norm and c.rl
            self.tg = self.d["target"].to(DEV)
            self.upstream = torch.ones(1, device=DEV)
            N.check(N.lib().mvn_softmax_ce_backward(
                self.out.data_ptr(), self.tg.data_ptr(), B, Q, c.S_out, 1.0 / max(B * c.S_out, 1),
                self.upstream.data_ptr(), self.bwd["dlogit"].data_ptr(), Q * self.Sp, self.Sp, c.pad, c.S_out + 1,
                _stream()), "mvn_softmax_ce_backward")
        b = self.bwd
        self.bb = N.BwdBuffers(*(_ptr(b.get(k)) for k in ("dx_a", "dx_b", "dfg", "dskip", "da1", "dlogit", "dctx")))

    def backward(self, **over):
        c = self.c
        a = dict(dims=self.dims, params=self.params, grads=self.grad_struct(), index=_ptr(self.index),
                 istride=self.istride, B=c.B, T=c.T, fb=self.fb, bb=self.bb,
                 out=_ptr(self.out) if (c.dout and c.S_out > 0) else None, dout=_ptr(self.dout) if c.S_out > 0 else None,
                 norm=int(c.norm), rl=int(c.rl))
        a.update(over)
        return getattr(N.lib(), ENTRY[self.entry][1])(a["dims"], a["params"], a["grads"], a["index"], a["istride"],
                                                      a["B"], a["T"], a["fb"], a["bb"], a["out"], a["dout"], a["norm"],
                                                      a["rl"], _stream())

    def snapshot(self, which):
        torch.cuda.synchronize()
        return {k: _bits(v) for k, v in which.items() if v is not None}

    def unchanged(self, snap, which, what):
        torch.cuda.synchronize()
        for k, v in which.items():
            if v is not None:
                assert torch.equal(_bits(v), snap[k]), (self.c, what, k, "changed")

    def everything(self):
        """every buffer the library could write or read"""
        d = dict(self.inputs)
        d.update(self.fwd)
        d["out"] = self.out
        if self.bwd is not None:
            d.update(self.bwd)
            d.update({"grad " + k: v for k, v in self.grads.items()})
            d["dout"] = self.dout
        return d

    def check_backward(self, what):
        c, ref, dev, g0 = self.c, self.d["ref"], self.d["dev"], self.d["g0"]
        self.g.check(f"{what}: backward")
        worst, at = 0.0, None
        for k, want in ref["grads"].items():
            got = self.grads[k].cpu()
            if want is None:
                # the last layer's residual conv reaches no output; no context, no context-conv gradient
                assert torch.equal(_bits(got), _bits(g0[k])), (c, what, k, "a gradient nothing flows into was written")
                continue
            e = _err(got.double() - g0[k].double(), want)
            bound = grad_bound(dev[k])
            if e / bound > worst or at is None:
                worst, at = e / bound, (k, e, bound)
            assert e < bound, (c, what, k, e, bound, dev[k])
        msg = f"backward {c} [{what}, form {N.lib().mvn_last_backward_form()}]: worst {at[1]:.1e} / {at[2]:.1e} ({at[0]})"
        if c.ctx:
            dctx = self.bwd["dctx"]
            assert bool(torch.isfinite(dctx).all()), (c, what, "dctx not finite")
            e, bound = _err(dctx[:, :, :c.T], ref["dctx"]), grad_bound(dev["dctx"])
            msg += f", dctx {e:.1e} / {bound:.1e}"
            assert e < bound, (c, what, "dctx", e, bound)
            # "(B, C, Tp), written in full": the columns from T on are zero
            assert bool((dctx[:, :, c.T:] == 0).all()), (c, what, "dctx columns >= T are not zero")
        print(msg)


def _full(c, what, entry="f32", form=None):
    """forward, backward, second backward, with every check of the module docstring"""
    r = Run(c, entry)
    assert r.forward() == N.MVN_OK, N.last_error()
    r.check_forward(what)
    saved = {k: v for k, v in r.fwd.items() if k != "z"}
    saved["out"] = r.out
    before = r.snapshot(saved)
    for round_ in ("first", "second"):
        r.prepare_backward()
        held = dict(r.inputs, out=r.out, dout=r.dout)
        snap = r.snapshot(held)
        assert r.backward() == N.MVN_OK, N.last_error()
        r.check_backward(f"{what}, {round_} backward")
        r.unchanged(snap, held, f"{what}, {round_} backward: input")
        if form is not None:
            assert N.lib().mvn_last_backward_form() == form, (c, what, N.lib().mvn_last_backward_form(), form)
    r.unchanged(before, saved, f"{what}: saved forward tensor after two backward passes")
    return r


# ---- 1. C = K = 64, Q = 256: the default forms on both sides of every scratch threshold ---------------------------
def _branches(c, cus):
    """What plan_forward / plan_backward (sequence.hip) decide for a C = K = 64, Q = 256 audio-only call
    (inequalities and constants: module docstring)"""
    pl = N.lib().mvn_padded_len
    Tp, Sp = pl(c.T), pl(c.S + 31)
    act = c.B * c.C * Tp
    z = "none"
    if act >= c.L * FS3_PACK_F:
        z = "layers"
    if act >= c.L * FSC_PACK_F + DS3_IMG_F:
        z = "fwd head"
    if act >= c.L * FSC_PACK_F + DS3_IMG_F + DS3_BWD_IMG_F:
        z = "bwd head"
    need = max((c.T + 31 + 511) // 512 * c.B, 2 * cus + c.B) * 128
    total = c.B * c.Q * Sp
    bias = "reserved" if need <= total // 2 else "small" if total // (128 * 64 + 128 * 128 + 128) >= c.B else "none"
    chunks = (c.S + 31 + 511) // 512
    head_ok = chunks * c.B * 256 * 257 <= c.B * 2 * c.C * Tp
    return z, bias, head_ok


# (layer_size, stack_size, B, T, wide index stride)  ->  z scratch, sc_bias, head_scratch_ok  on 256 CUs
# 10 x 3: RF = 3072; 3 x 2: RF = 16; 9 x 1: RF = 512
DEFAULT_ROWS = [
    ((10, 3, 1, 3072, False), ("none", "none", True)),          # T = RF, B = 1: one output column
    ((10, 3, 1, 3073, True), ("none", "none", True)),           # T = RF + 1
    ((10, 3, 7, 3074, False), ("fwd head", "none", True)),      # T = RF + 2, odd B: layer + forward head images only
    ((10, 3, 7, 3300, True), ("bwd head", "reserved", True)),   # ragged; all three image sets in z
    ((10, 3, 3, 3150, False), ("none", "small", True)),         # the small-tensor sc_bias path, form 3
    ((10, 3, 5, 4700, True), ("bwd head", "reserved", True)),   # S = 1629: four 512-column chunks
    ((3, 2, 1, 16, False), ("none", "none", False)),            # short stack, T = RF
    ((3, 2, 3, 17, True), ("none", "none", False)),             # T = RF + 1
    ((3, 2, 3, 18, False), ("none", "none", False)),            # T = RF + 2
    ((3, 2, 5, 333, True), ("none", "reserved", False)),        # ragged mid length
    ((3, 2, 3, 1500, False), ("layers", "reserved", False)),    # the layers' images only; three chunks
    ((3, 2, 5, 1700, True), ("bwd head", "reserved", False)),   # all images; four chunks, ragged
    ((3, 2, 1, 600, False), ("none", "reserved", False)),       # B = 1, two chunks
    ((9, 1, 1, 700, True), ("none", "small", True)),            # short stack WITH the head's slab scratch
]


@pytest.mark.parametrize("row,expect", DEFAULT_ROWS, ids=[str(r[0]) for r in DEFAULT_ROWS])
def test_default_forms_across_scratch_thresholds(row, expect):
    ls, ss, B, T, wide = row
    c = Case(ls, ss, 256, 64, 64, B, T, wide=wide)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    got = _branches(c, cus)
    assert cus != 256 or got == expect, (c, got, expect)
    # without a bias region the one-kernel form has no scratch: the generic layer loop (form 1) runs instead
    _full(c, f"z {got[0]}, sc_bias {got[1]}, head_scratch_ok {got[2]}", form=N.BWD_FORM_ONE if got[1] != "none" else
          N.BWD_FORM_GENERIC)


# ---- 2. the same shape under the kernel-form switches -----------------------------------------------------------------
class _Switch:
    def __init__(self, **env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.pop(k, None) for k in SWITCHES}
        os.environ.update(self.env)
        N.lib().mvn_reload_switches()

    def __exit__(self, *exc):
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in self.old.items() if v is not None})
        N.lib().mvn_reload_switches()


def _halves_fit(c, cus):
    """Whether the two fused halves (form 2) find their slabs at layer 0, the longest (sequence.hip halves_geometry):
    fused_bwd.h bwd_pass256_fits (chunks from fb_chunks, two workgroups per CU; 128 x 64 floats and 128 bias sums
    each) and bwd_dx_wgfg64_fits (one per CU; 128 x 128 floats each, behind the first half's), in BwdPlan::slab, which
    is da1 less the BwdPlan::bias2 reservation"""
    Sp = N.lib().mvn_padded_len(c.S + 31)
    bias2 = max((c.T + 31 + 511) // 512 * c.B, 2 * cus + c.B) * 128

    def chunks(t_lo, per_cu):
        tiles = -(-(c.T - (t_lo & ~31)) // 64)    # gemm_family.h: W2_T = 64
        chunk_tiles = max(1, -(-tiles // max(1, per_cu * cus // c.B)))
        return -(-tiles // chunk_tiles)

    a, b = chunks(c.A[1], 2) * c.B, chunks(c.A[0], 1) * c.B
    return a * 128 <= bias2 and a * 128 * 64 + b * 128 * 128 <= c.B * c.Q * Sp - bias2


ONE, HALVES, GENERIC = N.BWD_FORM_ONE, N.BWD_FORM_HALVES, N.BWD_FORM_GENERIC
SWITCH_CASES = [
    ({}, ONE),
    ({"MOVENET_HIP_NO_FUSED_FORWARD": "1"}, ONE),
    ({"MOVENET_HIP_FORWARD_MFMA": "f32"}, ONE),
    ({"MOVENET_HIP_FORWARD_TILE": "1"}, ONE),
    ({"MOVENET_HIP_BWD_FORM": "split"}, HALVES),
    ({"MOVENET_HIP_NO_FUSED_BACKWARD": "1"}, GENERIC),
]


SMALL, LARGE = (3, 2, 5, 333), (3, 2, 7, 6000)
# SMALL runs under every switch; the halves' slabs do not fit its da1 (_halves_fit: they need B T > 2 x 64 x CUs
# columns), so BWD_FORM=split falls to the generic layer loop there (form 1, asserted from the inequality).  LARGE is
# the smallest kind of shape that reaches form 2, under the three settings that choose the BACKWARD's form.  It is
# not run under the forward's switches, for a reason that lies in the reference, not in the kernels: its head holds
# 10.7 M leaky-ReLU inputs, a few of them closer to zero than fp32 resolves, and lrelu' jumps from 0.01 to 1 there.
# The float32 CPU oracle itself lands 2.0e-3 from float64 on the causal conv's gradient of this case -- beyond
# grad_bound's cap of 3e-4 -- and so does any forward that rounds one such input to the other side: measured 7.9e-4
# with NO_FUSED_FORWARD=1 and FORWARD_MFMA=f32 (identical: same saved signs), < 4e-5 with the default and the tile
# forward.  The forward's switches are cross-checked where the reference is within its own cap (SMALL: dev <= 2.4e-6).
SWITCH_ROWS = [(SMALL, i) for i in range(6)] + [(LARGE, i) for i in (0, 4, 5)]


@pytest.mark.parametrize("shape,which", SWITCH_ROWS,
                         ids=[f"{s}-{','.join(SWITCH_CASES[i][0]) or 'default'}" for s, i in SWITCH_ROWS])
def test_kernel_form_switches(shape, which):
    env, form = SWITCH_CASES[which]
    ls, ss, B, T = shape
    c = Case(ls, ss, 256, 64, 64, B, T, wide=True)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert _branches(c, cus)[1] == "reserved"
    assert cus != 256 or _halves_fit(c, cus) == (shape == LARGE)
    if form == HALVES and not _halves_fit(c, cus):
        form = GENERIC
    with _Switch(**env):
        _full(c, ",".join(f"{k[12:]}={v}" for k, v in env.items()) or "default", form=form)


# ---- 3. generic dims, conditioning, dense input -------------------------------------------------------------------------
GENERIC_DIMS = [(100, 24, 40), (256, 128, 128), (257, 64, 64), (64, 64, 32)]


@pytest.mark.parametrize("B,T,wide", [(3, 200, True), (1, 77, False)])
@pytest.mark.parametrize("Q,C,K", GENERIC_DIMS)
def test_generic_dims(Q, C, K, B, T, wide):
    # K != 64 or C != 64: the generic layer loop; (257, 64, 64): the fused layers with the generic head (form 3 / 1
    # by the scratch, not asserted: Q = 257 moves every threshold of section 1)
    _full(Case(3, 2, Q, C, K, B, T, wide=wide), "generic dims", form=None if (C, K) == (64, 64) else N.BWD_FORM_GENERIC)


@pytest.mark.parametrize("ld", ["tight", "wide"])
@pytest.mark.parametrize("Q,C,K,B,T", [(256, 64, 64, 3, 333), (256, 64, 64, 5, 1700), (100, 24, 40, 3, 200),
                                       (256, 64, 64, 1, 20)])
def test_conditioned(Q, C, K, B, T, ld):
    _full(Case(3, 2, Q, C, K, B, T, ctx=ld, wide=(ld == "wide")), f"ctx_ld {ld}")


@pytest.mark.parametrize("Q,C,K,B,T,ctx", [(256, 64, 64, 3, 333, None), (100, 24, 40, 3, 200, None),
                                           (64, 64, 64, 2, 150, "wide")])
def test_dense_input(Q, C, K, B, T, ctx):
    r = _full(Case(3, 2, Q, C, K, B, T, dense=True, ctx=ctx), "dense input, index = NULL")
    assert r.index is None and r.dense_ld > T


# ---- 4. flags ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,C,K", [(256, 64, 64), (100, 24, 40)])
@pytest.mark.parametrize("norm,rl,dout", [(False, False, True), (False, True, True), (True, False, True),
                                          (True, True, True), (True, True, False)])
def test_flags(norm, rl, dout, Q, C, K):
    _full(Case(3, 2, Q, C, K, 3, 100, wide=True, norm=norm, rl=rl, dout=dout), "flags")


@pytest.mark.parametrize("Q,C,K", [(256, 64, 64), (100, 24, 40)])
@pytest.mark.parametrize("norm", [False, True])
def test_empty_output(norm, Q, C, K):
    """T == RF with remove_last: S_out = 0.  Both calls return MVN_OK with out = NULL (and dout = NULL or not); the
    forward still fills the saved tensors (a saved forward of RF samples primes a generator), writes nothing to
    `out`; the backward launches nothing: gradients, scratch and every other buffer keep their bits."""
    c = Case(3, 2, Q, C, K, 3, 16, norm=norm, rl=True)
    assert c.S_out == 0
    r = Run(c)
    assert r.forward(out=None) == N.MVN_OK, N.last_error()
    r.check_forward("S_out = 0")
    r.prepare_backward()
    nothing = r.g.new((1,), NAN, "dout of no elements")
    snap = r.snapshot(r.everything())
    for dout in (None, nothing.data_ptr()):
        assert r.backward(out=None, dout=dout) == N.MVN_OK, N.last_error()
        r.g.check("S_out = 0: backward")
        r.unchanged(snap, r.everything(), "S_out = 0: backward")


# ---- 5. save = 0 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,C,K,B,T,env", [(256, 64, 64, 5, 1700, {}), (256, 64, 64, 3, 333, {}), (100, 24, 40, 3, 200, {}),
                                           (256, 64, 64, 3, 333, {"MOVENET_HIP_NO_FUSED_FORWARD": "1"}),
                                           (256, 64, 64, 3, 333, {"MOVENET_HIP_FORWARD_TILE": "1"})])
def test_save_0_equals_save_1(Q, C, K, B, T, env):
    """th = sg = NULL and two acts planes.  forward_impl chooses every kernel from the dims, the lengths and the
    switches, never from `save`; `save` only turns the th / sg stores off and makes the layers alternate between two
    planes.  Same kernels, same launch geometry, same order of every sum: `out` is equal BIT FOR BIT."""
    c = Case(3, 2, Q, C, K, B, T, wide=True, norm=True, rl=True)
    with _Switch(**env):
        a, b = Run(c, save=True), Run(c, save=False)
        assert b.fb.th is None and b.fb.sg is None and b.fwd["acts"].shape[0] == 2
        for r in (a, b):
            assert r.forward() == N.MVN_OK, N.last_error()
        a.check_forward("save = 1")
        b.check_forward("save = 0")
    assert torch.equal(_bits(a.out), _bits(b.out)), (c, env)


# ---- 6. bf16 and f16 --------------------------------------------------------------------------------------------------
# test_bf16_train_gpu.RAGGED's shapes; t_rf_plus_1: da1 is too small for the slabs, they go to the forward's z
BF16 = {"b3_t_not_64": (10, 3, 256, 3, 3170), "t_rf_plus_1": (10, 3, 256, 2, 3073), "stack_2x2": (2, 2, 256, 2, 300),
        "dilation_past_span": (10, 1, 64, 2, 1025)}


@functools.lru_cache(maxsize=None)
def _emulation(key):
    c = Case(*key[:7], norm=key[9], rl=key[10], dout=key[11])
    d = _data(key)
    return _oracle(c, d["sd"], d["x"], None, d["up"], d["target"], torch.float32, logits_fn=E.logits)


@pytest.mark.parametrize("name", sorted(BF16))
def test_bf16_entry_points(name):
    from test_bf16_train_gpu import _check_grads
    ls, ss, Q, B, T = BF16[name]
    c = Case(ls, ss, Q, 64, 64, B, T, wide=True, rl=True)
    if name == "t_rf_plus_1":   # sequence.hip plan_backward, `!layer_fits() && fwd->z`: B Q Sp / 24704 < B
        assert c.B * c.Q * N.lib().mvn_padded_len(c.S + 31) // 24704 < c.B
    r = Run(c, "bf16")
    ref, emu = r.d["ref"], _emulation(c.key())
    assert r.forward() == N.MVN_OK, N.last_error()
    r.check_forward("bf16", values=False, tol=float("inf"))   # bands, finiteness, acts[L]; the values: below
    e_got, e_emu = _err(r.out, ref["out"]), _err(emu["out"], ref["out"])
    print(f"bf16 {c}: logits {e_got:.2e}, emulation {e_emu:.2e}")
    assert e_got <= 2 * e_emu, (e_got, e_emu)
    saved = {k: v for k, v in r.fwd.items() if k != "z"}
    before = r.snapshot(saved)
    want = {k: v for k, v in ref["grads"].items() if v is not None}
    for round_ in ("first", "second"):
        r.prepare_backward()
        held = dict(r.inputs, out=r.out, dout=r.dout)
        snap = r.snapshot(held)
        assert r.backward() == N.MVN_OK, N.last_error()
        assert N.lib().mvn_last_backward_form() == N.BWD_FORM_BF16
        r.g.check(f"bf16 {round_} backward")
        got = {k: (r.grads[k].double() - r.d["g0"][k].double().to(DEV)).float() for k in want}
        worst, emu_min = _check_grads(got, want, {k: emu["grads"][k] for k in want}, f"{name} {round_}")
        print(f"bf16 {c} {round_} backward: worst cosine {worst:.5f} (emulation {emu_min:.5f})")
        for k, v in ref["grads"].items():
            if v is None:
                assert torch.equal(_bits(r.grads[k].cpu()), _bits(r.d["g0"][k])), (c, k)
        r.unchanged(snap, held, f"bf16 {round_} backward: input")
    r.unchanged(before, saved, "bf16: saved forward tensor after two backward passes")


@pytest.mark.parametrize("C,K,ctx", [(16, 16, None), (64, 32, None), (64, 64, "tight")])
def test_bf16_unsupported_writes_nothing(C, K, ctx):
    r = Run(Case(3, 2, 256, C, K, 3, 100, ctx=ctx), "bf16")
    r.prepare_backward()
    snap = r.snapshot(r.everything())
    assert r.forward() == N.MVN_ERR_UNSUPPORTED and N.last_error() != ""
    assert r.backward() == N.MVN_ERR_UNSUPPORTED and N.last_error() != ""
    r.g.check("refused bf16 calls")
    r.unchanged(snap, r.everything(), "refused bf16 calls")


@pytest.mark.parametrize("Q,C,K,B,T", [(256, 64, 64, 3, 333), (256, 128, 128, 3, 200), (100, 24, 40, 1, 77)])
def test_f16_forward_poisoned(Q, C, K, B, T):
    r = Run(Case(3, 2, Q, C, K, B, T, wide=True), "f16")
    assert r.forward() == N.MVN_OK, N.last_error()
    r.check_forward("f16", tol=FP16_TOL)


# ---- 7. refusals --------------------------------------------------------------------------------------------------------
def _fb(r, **over):
    f = {k: getattr(r.fb, k) for k, _ in N.FwdBuffers._fields_}
    f.update(over)
    return N.FwdBuffers(*(f[k] for k, _ in N.FwdBuffers._fields_))


def _bb(r, **over):
    f = {k: getattr(r.bb, k) for k, _ in N.BwdBuffers._fields_}
    f.update(over)
    return N.BwdBuffers(*(f[k] for k, _ in N.BwdBuffers._fields_))


def _without_ctx_params(r):
    p = N.Params()
    for k, _ in N.Params._fields_:
        setattr(p, k, getattr(r.params, k))
    p.ctx_gate_b = None
    return p


@pytest.mark.parametrize("Q,C,K", [(256, 64, 64), (100, 24, 40)])
def test_refusals_leave_every_buffer_untouched(Q, C, K):
    c = Case(3, 2, Q, C, K, 3, 100, ctx="wide", wide=True, norm=True)
    r = Run(c)
    r.prepare_backward()
    snap = r.snapshot(r.everything())
    bad = N.MVN_ERR_BAD_ARG
    fwd_calls = [
        (dict(index=None), bad), (dict(istride=c.T - 1), bad), (dict(out=None), bad), (dict(params=None), bad),
        (dict(fb=None), bad), (dict(B=-1), bad), (dict(T=0), bad), (dict(dims=None), bad),
        (dict(T=c.RF - 1, istride=c.T), N.MVN_ERR_TOO_SHORT),
        (dict(dims=N.make_dims(3, 2, Q, 0, K)), N.MVN_ERR_BAD_DIMS),
        (dict(fb=_fb(r, ctx_ld=c.T - 1)), bad), (dict(fb=_fb(r, ctx_ld=0)), bad),
        (dict(params=_without_ctx_params(r)), bad),
    ] + [(dict(fb=_fb(r, **{k: None})), bad) for k in ("acts", "th", "sg", "z", "skip", "a1")]
    for over, code in fwd_calls:
        assert r.forward(**over) == code, (over, N.last_error())
        assert N.last_error() != ""
    r.g.check("refused forward calls")
    r.unchanged(snap, r.everything(), "refused forward calls")
    assert r.forward() == N.MVN_OK, N.last_error()   # the call these were variations of runs
    r.check_forward("after the refusals")
    r.prepare_backward()
    snap = r.snapshot(r.everything())
    bwd_calls = [
        (dict(index=None), bad), (dict(istride=c.T - 1), bad), (dict(out=None), bad), (dict(params=None), bad),
        (dict(grads=None), bad), (dict(fb=None), bad), (dict(bb=None), bad), (dict(B=-1), bad), (dict(dims=None), bad),
        (dict(T=c.RF - 1), N.MVN_ERR_TOO_SHORT), (dict(dims=N.make_dims(3, 2, Q, C, 0)), N.MVN_ERR_BAD_DIMS),
        (dict(fb=_fb(r, ctx_ld=c.T - 1)), bad), (dict(grads=r.grad_struct(without=("ctx_filter_w",))), bad),
        (dict(grads=r.grad_struct(without=("ctx_gate_b",))), bad),
    ] + [(dict(fb=_fb(r, **{k: None})), bad) for k in ("acts", "th", "sg", "skip", "a1")] \
      + [(dict(bb=_bb(r, **{k: None})), bad) for k in ("dx_a", "dx_b", "dfg", "dskip", "da1", "dlogit", "dctx")]
    for over, code in bwd_calls:
        assert r.backward(**over) == code, (over, N.last_error())
        assert N.last_error() != ""
    r.g.check("refused backward calls")
    r.unchanged(snap, r.everything(), "refused backward calls")
    assert r.backward() == N.MVN_OK, N.last_error()
    r.check_backward("after the refusals")


def test_dense_stride_refusals():
    c = Case(3, 2, 100, 24, 40, 2, 64, dense=True)
    r = Run(c)
    r.prepare_backward()
    snap = r.snapshot(r.everything())
    assert r.forward(fb=_fb(r, dense_ld=c.T - 1)) == N.MVN_ERR_BAD_ARG
    assert r.backward(fb=_fb(r, dense_ld=c.T - 1)) == N.MVN_ERR_BAD_ARG
    r.g.check("refused dense calls")
    r.unchanged(snap, r.everything(), "refused dense calls")
