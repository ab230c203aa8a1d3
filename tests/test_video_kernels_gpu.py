"""GPU: the video encoder, the learned up-sampler and the context transpose through the C ABI, against float64 torch.

``mvn_upsample_video``, ``mvn_upsample_video_backward``, ``mvn_upsample_video_scratch_floats`` (csrc/video.hip) and
``mvn_transpose_context`` (csrc/generate.hip), called directly on synthetic data.  The reference is
``conv3d`` + 3 x ``conv_transpose1d(stride=10)`` in float64 on the CPU with autograd; the upstream gradient is seeded
standard-normal noise and the weights are scaled so that every activation and gradient is O(1) (conv weight
/ sqrt(4096 cin), up-sampler weights / sqrt(C)): a wrong term shows at full size.

What is covered that nothing else runs: ``cin`` > 1 (``video_conv_kernel`` with one frame per workgroup, up to 128 KB
of LDS), frame counts that leave the four-frame groups partly empty, each forward stage on its own, the generic
up-sampler forms at C = 24 / 128 / 256 / 1, ``up_bwd64_kernel`` with SEVERAL tiles per workgroup (proved from the
sizing function, not assumed from the CU count) and with its atomics fall-back, accumulation into the gradients,
leading dimensions above 1000 F, and NaN in every column the library has no business reading.

Every buffer handed to the library is the front of a larger allocation with a sentinel band behind it (``_Guard``),
checked after each call.  Bounds (max |err| / max |ref| per tensor): forward stages 1e-5 (the bound of fixture G7),
gradients 2e-5 ("fp32 sums in another order", test_conditioning_gpu.py); where the SAME reference computed in fp32 on
the CPU deviates from float64 by more than 5e-6 for a tensor, that tensor's bound is four times that deviation, never
above 3e-4 (helpers.grad_bound).  No bound comes from the kernels' own output.

Largest errors seen on an MI355X (256 CUs), per group of cases (the file runs in 6 s):
  forward stages, C = 64 ............................. 5.2e-7 (ctx; B 40, F 3, cin 2)
  forward stages, C = 16 / 24 / 1 / 128 / 256 ........ 7.3e-7 (u1; C 256, F 4)
  backward C = 64, slab form ......................... 5.0e-7 (up_w0 gradient; B 3, F 7, cin 8), d_* 3.3e-7
  backward C = 64, no scratch / one float short ...... 5.5e-7 (up_w2 gradient; B 64, F 2), d_* 3.0e-7
  backward, generic forms ............................ 1.7e-6 (d_u2; C 128), gradients 1.4e-6 (conv_w; C 128)
The largest bound grad_bound gave was 5.3e-5 (the last layer's bias gradient at config 3's shape, fp32 on the CPU
1.3e-5 from float64); the kernels were at 1.8e-7 there.

Defects this file was written against, all fixed in csrc/video.hip (host side): with a scratch one float short of
the sizing function's answer the two short layers still wrote their slabs into it and only the last layer took the
atomics (test_slab_form_and_atomics_form failed on its first run); the backward did not look at the up-sampler
weight pointers at all, and found a NULL gradient pointer of layer 0 or 1 only after the later layers had been
launched (test_argument_checks; seen in the code, never run in that state); a dctx_ld that is not a multiple of 4
reached up_bwd64_kernel's 16-byte loads (now refused, test_c64_backward_refuses_...).
"""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as Fn

from helpers import BAND, DEV, SENTINEL, _Guard, grad_bound
from movenet_amd import _native as N

pytestmark = pytest.mark.gpu
NAN = float("nan")
TOL_FWD = 1e-5
PNAMES = ("conv_w", "conv_b", "up_w0", "up_b0", "up_w1", "up_b1", "up_w2", "up_b2")
SLAB_FLOATS = 640 * 64 + 64        # one workgroup's weight-gradient slab and its 64 bias sums (C = 64)
_V3 = ctypes.c_void_p * 3


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _err(got, want):
    return ((got.double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-30)).item()


def _dims(C):
    return N.make_dims(2, 2, 64, C, C)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _vstruct(t):
    """mvn_video_params / mvn_video_grads of a {name: device tensor or None}"""
    return N.VideoParams(_ptr(t["conv_w"]), _ptr(t["conv_b"]),
                         _V3(_ptr(t["up_w0"]), _ptr(t["up_w1"]), _ptr(t["up_w2"])),
                         _V3(_ptr(t["up_b0"]), _ptr(t["up_b1"]), _ptr(t["up_b2"])))


def _wide(n):
    """a leading dimension above n: the next multiple of 64 past it, plus 64"""
    return N.lib().mvn_padded_len(n + 1) + 64


# ---- data and the reference --------------------------------------------------------------------------------------
def _reference(p, video, dctx, dtype):
    q = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in p.items()}
    x = Fn.conv3d(video.to(dtype).permute(0, 4, 1, 2, 3), q["conv_w"], q["conv_b"]).squeeze(-1).squeeze(-1)
    stages = [x]
    for i in range(3):
        stages.append(Fn.conv_transpose1d(stages[-1], q[f"up_w{i}"], q[f"up_b{i}"], stride=10))
    for s in stages[:3]:
        s.retain_grad()
    stages[3].backward(dctx.to(dtype))
    out = dict(zip(("enc", "u1", "u2", "ctx"), (s.detach() for s in stages)))
    out.update(d_enc=stages[0].grad, d_u1=stages[1].grad, d_u2=stages[2].grad)
    out.update({"g_" + k: v.grad for k, v in q.items()})
    return out


@functools.lru_cache(maxsize=None)
def _case(B, F, C, cin):
    """Seeded inputs of a case, its float64 reference (built once per module: the config-3 shape's is ~130 MB) and,
    per tensor, how far the same computation in fp32 on the CPU lands from it."""
    g = torch.Generator().manual_seed(100003 * B + 1009 * F + 17 * C + cin)

    def r(*shape):
        return torch.randn(*shape, generator=g)

    p = {"conv_w": r(C, cin, 1, 64, 64) / math.sqrt(4096 * cin), "conv_b": 0.5 * r(C)}
    for i in range(3):
        p[f"up_w{i}"] = r(C, C, 10) / math.sqrt(C)
        p[f"up_b{i}"] = 0.5 * r(C)
    video = r(B, F, 64, 64, cin)
    dctx = r(B, C, 1000 * F)
    g0 = {k: r(*v.shape) for k, v in p.items()}   # what the gradient buffers hold before the call
    ref = _reference(p, video, dctx, torch.float64)
    ref32 = _reference(p, video, dctx, torch.float32)
    dev = {k: _err(ref32[k], ref[k]) for k in ref}
    return p, video, dctx, g0, ref, dev


# ---- the library ---------------------------------------------------------------------------------------------------
def _forward(B, F, C, cin, ctx_ld, guard):
    """-> device params, video, enc, u1, u2 (NaN in their padding columns), ctx (sentinel past 1000 F)"""
    lib = N.lib()
    p, video, _, _, _, _ = _case(B, F, C, cin)
    pd = {k: guard.put(v, k) for k, v in p.items()}
    vd = guard.put(video, "video")
    pl = lib.mvn_padded_len
    enc = guard.new((B, C, pl(F)), NAN, "enc")
    u1 = guard.new((B, C, pl(10 * F)), NAN, "u1")
    u2 = guard.new((B, C, pl(100 * F)), NAN, "u2")
    ctx = guard.new((B, C, ctx_ld), SENTINEL, "ctx")
    N.check(lib.mvn_upsample_video(_dims(C), _vstruct(pd), vd.data_ptr(), B, F, cin, enc.data_ptr(), u1.data_ptr(),
                                   u2.data_ptr(), ctx.data_ptr(), ctx_ld, _stream()), "mvn_upsample_video")
    guard.check("mvn_upsample_video")
    return pd, vd, enc, u1, u2, ctx


def _check_forward(case, enc, u1, u2, ctx):
    B, F, C, cin = case
    ref = _case(*case)[4]
    worst = {}
    for name, got, n in (("enc", enc, F), ("u1", u1, 10 * F), ("u2", u2, 100 * F), ("ctx", ctx, 1000 * F)):
        valid = got[:, :, :n]
        assert bool(torch.isfinite(valid).all()), (case, name)
        worst[name] = _err(valid, ref[name])
        # what lies behind the valid columns is the caller's: NaN stays NaN, the sentinel stays the sentinel
        pad = got[:, :, n:]
        if name == "ctx":
            assert bool((pad == SENTINEL).all()), (case, "columns of ctx past 1000 F were written")
        else:
            assert bool(torch.isnan(pad).all()), (case, name, "padding columns were written")
    print(f"forward {case}: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for name, e in worst.items():
        assert e < TOL_FWD, (case, name, e)
    return worst


def _scratch_wgs(B, F, C=64):
    """workgroups per sequence of the last up-sampler layer's backward launch, from the sizing function"""
    n = int(N.lib().mvn_upsample_video_scratch_floats(_dims(C), B, F))
    assert n % (B * SLAB_FLOATS) == 0, n
    return n, n // (B * SLAB_FLOATS)


def _backward(case, guard, pd, vd, enc, u1, u2, dctx_ld, mode="slab"):
    """mode: 'slab' (the scratch the sizing function asks for), 'null' (no scratch), 'short' (one float short)
    -> gradients (pre-filled with g0), d_u2, d_u1, d_enc (pre-filled with NaN)"""
    lib = N.lib()
    B, F, C, cin = case
    _, _, dctx, g0, _, _ = _case(*case)
    d = guard.new((B, C, dctx_ld), NAN, "dctx")   # NaN in the columns past 1000 F
    d[:, :, :1000 * F] = dctx.to(DEV)
    grads = {k: guard.put(v, "grad " + k) for k, v in g0.items()}
    d_u2, d_u1, d_enc = (guard.new(tuple(t.shape), NAN, n) for t, n in ((u2, "d_u2"), (u1, "d_u1"), (enc, "d_enc")))
    n = int(lib.mvn_upsample_video_scratch_floats(_dims(C), B, F))
    scratch = None if mode == "null" else guard.new((max(n, 1),), SENTINEL, "scratch")
    given = {"slab": n, "null": 0, "short": n - 1}[mode]
    N.check(lib.mvn_upsample_video_backward(
        _dims(C), _vstruct(pd), _vstruct(grads), vd.data_ptr(), B, F, cin, enc.data_ptr(), u1.data_ptr(),
        u2.data_ptr(), d.data_ptr(), dctx_ld, d_u2.data_ptr(), d_u1.data_ptr(), d_enc.data_ptr(), _ptr(scratch),
        given, _stream()), "mvn_upsample_video_backward")
    guard.check(f"mvn_upsample_video_backward ({mode})")
    if mode == "short":
        assert n > 0 and bool((scratch == SENTINEL).all()), "a scratch one float too small was written to"
    return grads, d_u2, d_u1, d_enc


def _check_backward(case, what, grads, d_u2, d_u1, d_enc):
    B, F, C, cin = case
    _, _, _, g0, ref, dev = _case(*case)
    worst = {}
    for name, got, n in (("d_u2", d_u2, 100 * F), ("d_u1", d_u1, 10 * F), ("d_enc", d_enc, F)):
        valid = got[:, :, :n]
        assert bool(torch.isfinite(valid).all()), (case, what, name)
        worst[name] = _err(valid, ref[name])
    for k in PNAMES:
        assert bool(torch.isfinite(grads[k]).all()), (case, what, k)
        # accumulated into: the buffer held g0
        worst["g_" + k] = _err(grads[k].double().cpu() - g0[k].double(), ref["g_" + k])
    print(f"backward {case} {what}: " + " ".join(f"{k} {v:.2e}/{grad_bound(dev[k]):.1e}" for k, v in worst.items()))
    for k, e in worst.items():
        assert e < grad_bound(dev[k]), (case, what, k, e, dev[k])
    return worst


# ---- 1. forward, each stage on its own -------------------------------------------------------------------------
# (B, F, C, cin, wide ctx_ld): C 64 / 16 / 24 / 1 / 128 / 256, cin 1 / 2 / 3 / 8 (cin > 1: one frame per workgroup,
# channel-interleaved pixel reads; 8: 128 KB of LDS), F 1 / 3 / 4 / 5 / 7 / 32 (3, 5, 7 leave the four-frame groups of
# cin = 1 partly empty), B 1 / 3 / 8
FORWARD_CASES = [
    (1, 1, 64, 1, False), (3, 3, 64, 2, True), (8, 4, 64, 3, False), (3, 7, 64, 8, True), (8, 32, 64, 1, False),
    (1, 5, 64, 1, True), (3, 5, 16, 8, True), (8, 3, 16, 1, False), (1, 7, 24, 3, True), (3, 4, 24, 1, False),
    (3, 1, 1, 2, False), (1, 7, 1, 1, True), (1, 5, 128, 1, True), (3, 1, 128, 3, False), (1, 3, 256, 3, False),
    (1, 4, 256, 1, True),
]


@pytest.mark.parametrize("B,F,C,cin,wide", FORWARD_CASES)
def test_forward_stages_vs_float64(B, F, C, cin, wide):
    guard = _Guard()
    ctx_ld = _wide(1000 * F) if wide else 1000 * F
    _, _, enc, u1, u2, ctx = _forward(B, F, C, cin, ctx_ld, guard)
    _check_forward((B, F, C, cin), enc, u1, u2, ctx)


# ---- 2. backward against float64 autograd -----------------------------------------------------------------------
# C = 64 (up_bwd64_kernel).  multi: a workgroup walks several 32-step tiles of the last layer -- B = 64, F = 2 (7
# tiles; on 256 CUs two per workgroup, the last workgroup holding one: the `break`), config 3's own B = 8, F = 32
# (100 tiles, four per workgroup), B = 40, F = 3 (10 tiles).  The others have one tile per workgroup: F = 1 (layers
# of 1, 10 and 100 steps: a lone partial tile; three tiles and a 4-step tail), odd F, cin 1 / 3 / 8.
BWD64_CASES = [
    (1, 1, 64, 1, False), (4, 3, 64, 3, False), (3, 7, 64, 8, False), (1, 5, 64, 1, False),
    (64, 2, 64, 1, True), (8, 32, 64, 1, True), (40, 3, 64, 2, True),
]


def _assert_tiling(B, F, multi):
    n, wgs = _scratch_wgs(B, F)
    tiles = -(-100 * F // 32)
    if multi:
        assert wgs < tiles, f"B {B} F {F}: {wgs} workgroups for {tiles} tiles -- not the several-tiles path"
    else:
        assert wgs == tiles, (B, F, wgs, tiles)
    return wgs, tiles


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("B,F,C,cin,multi", BWD64_CASES)
def test_backward_c64_vs_float64(B, F, C, cin, multi, wide):
    case = (B, F, C, cin)
    wgs, tiles = _assert_tiling(B, F, multi)
    guard = _Guard()
    pd, vd, enc, u1, u2, ctx = _forward(B, F, C, cin, 1000 * F, guard)
    _check_forward(case, enc, u1, u2, ctx)
    dctx_ld = _wide(1000 * F) if wide else 1000 * F
    out = _backward(case, guard, pd, vd, enc, u1, u2, dctx_ld, "slab")
    _check_backward(case, f"slab, {wgs} workgroups / {tiles} tiles, dctx_ld {dctx_ld}", *out)


# generic forms (UpOp / UpDxOp / UpWgOp through gemm_wx_kernel / wgrad_kernel): 10 C = 160 (not a multiple of 64: the
# scatter epilogue's row guard), 240, 1280 (20 row blocks)
BWD_GENERIC_CASES = [
    (3, 3, 16, 1), (2, 5, 16, 3), (2, 5, 24, 1), (3, 1, 24, 3), (1, 7, 24, 8), (2, 3, 128, 1), (1, 5, 128, 3),
]


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("B,F,C,cin", BWD_GENERIC_CASES)
def test_backward_generic_forms_vs_float64(B, F, C, cin, wide):
    case = (B, F, C, cin)
    assert N.lib().mvn_upsample_video_scratch_floats(_dims(C), B, F) == 0
    guard = _Guard()
    pd, vd, enc, u1, u2, ctx = _forward(B, F, C, cin, 1000 * F, guard)
    _check_forward(case, enc, u1, u2, ctx)
    dctx_ld = _wide(1000 * F) if wide else 1000 * F
    out = _backward(case, guard, pd, vd, enc, u1, u2, dctx_ld, "slab")
    _check_backward(case, f"generic, dctx_ld {dctx_ld}", *out)


# ---- 3. the slab form against the atomics form (C = 64) ------------------------------------------------------------
@pytest.mark.parametrize("B,F,cin,multi", [(4, 3, 3, False), (64, 2, 1, True), (1, 1, 1, False)])
def test_slab_form_and_atomics_form(B, F, cin, multi):
    case = (B, F, 64, cin)
    wgs, tiles = _assert_tiling(B, F, multi)
    guard = _Guard()
    pd, vd, enc, u1, u2, ctx = _forward(B, F, 64, cin, 1000 * F, guard)
    runs = {}
    for mode in ("slab", "null", "short", "slab"):
        out = _backward(case, guard, pd, vd, enc, u1, u2, 1000 * F, mode)
        _check_backward(case, f"{mode}, {wgs} workgroups / {tiles} tiles", *out)
        runs.setdefault(mode, []).append(out)
    # the slab form sums in a fixed order: twice the same bits (nothing bitwise is asked of the atomics form)
    (ga, *da), (gb, *db) = runs["slab"]
    for k in PNAMES[1:]:   # (conv_w is added to with atomics by one workgroup per sequence)
        assert torch.equal(ga[k], gb[k]), (case, k)
    for a, b, n in zip(da, db, (100 * F, 10 * F, F)):
        assert torch.equal(a[:, :, :n], b[:, :, :n])


def test_scratch_sizing():
    lib = N.lib()
    for C in (1, 16, 24, 63, 65, 128, 256):
        assert lib.mvn_upsample_video_scratch_floats(_dims(C), 8, 32) == 0
    d = _dims(64)
    for B, F in ((0, 4), (-1, 4), (4, 0), (4, -3)):
        assert lib.mvn_upsample_video_scratch_floats(d, B, F) == 0
    assert lib.mvn_upsample_video_scratch_floats(None, 4, 4) == 0
    n, wgs = _scratch_wgs(8, 32)
    assert n > 0 and 1 <= wgs <= 100
    assert _scratch_wgs(1, 1) == (4 * SLAB_FLOATS, 4)   # 100 steps: four tiles, never more workgroups than tiles


# ---- 4. argument checks ------------------------------------------------------------------------------------------
def _refused(rc, code=N.MVN_ERR_BAD_ARG):
    assert rc == code, (rc, N.last_error())
    assert N.last_error() != ""


class _Call:
    """A valid call of both entry points at B = 1, F = 1 whose every output holds the sentinel"""

    def __init__(self, C):
        lib = N.lib()
        self.C, self.guard = C, _Guard()
        g = torch.Generator().manual_seed(5)
        shapes = {"conv_w": (C, 1, 1, 64, 64), "conv_b": (C,)}
        for i in range(3):
            shapes[f"up_w{i}"], shapes[f"up_b{i}"] = (C, C, 10), (C,)
        self.p = {k: self.guard.put(torch.randn(*s, generator=g) * 0.05, k) for k, s in shapes.items()}
        self.g = {k: self.guard.new(s, SENTINEL, "grad " + k) for k, s in shapes.items()}
        self.video = self.guard.put(torch.randn(1, 1, 64, 64, 1, generator=g), "video")
        pl = lib.mvn_padded_len
        new = self.guard.new
        self.fwd_out = dict(enc=new((1, C, pl(1)), SENTINEL), u1=new((1, C, pl(10)), SENTINEL),
                            u2=new((1, C, pl(100)), SENTINEL), ctx=new((1, C, 1024), SENTINEL))
        self.acts = dict(enc=new((1, C, pl(1)), 0.25), u1=new((1, C, pl(10)), 0.25), u2=new((1, C, pl(100)), 0.25))
        self.dctx = new((1, C, 1024), 0.5, "dctx")
        self.bwd_out = dict(d_u2=new((1, C, pl(100)), SENTINEL), d_u1=new((1, C, pl(10)), SENTINEL),
                            d_enc=new((1, C, pl(1)), SENTINEL))
        self.n_scratch = int(lib.mvn_upsample_video_scratch_floats(_dims(C), 1, 1))
        self.scratch = new((max(self.n_scratch, 1),), SENTINEL, "scratch")

    def forward(self, dims="own", vp=None, video="own", batch=1, frames=1, cin=1, ctx_ld=1024, **bufs):
        o = {k: _ptr(v) for k, v in self.fwd_out.items()}
        o.update(bufs)
        return N.lib().mvn_upsample_video(
            _dims(self.C) if dims == "own" else dims, _vstruct(self.p) if vp is None else vp,
            self.video.data_ptr() if video == "own" else video, batch, frames, cin, o["enc"], o["u1"], o["u2"],
            o["ctx"], ctx_ld, _stream())

    def backward(self, dims="own", vp=None, vg=None, video="own", batch=1, frames=1, cin=1, dctx="own", dctx_ld=1024,
                 **bufs):
        o = {k: _ptr(v) for k, v in {**self.acts, **self.bwd_out}.items()}
        o.update(bufs)
        return N.lib().mvn_upsample_video_backward(
            _dims(self.C) if dims == "own" else dims, _vstruct(self.p) if vp is None else vp,
            _vstruct(self.g) if vg is None else vg, self.video.data_ptr() if video == "own" else video, batch, frames,
            cin, o["enc"], o["u1"], o["u2"], self.dctx.data_ptr() if dctx == "own" else dctx, dctx_ld, o["d_u2"],
            o["d_u1"], o["d_enc"], self.scratch.data_ptr(), self.n_scratch, _stream())

    def without(self, which, key):
        t = dict(self.p if which == "p" else self.g)
        t[key] = None
        return _vstruct(t)

    def untouched(self, what):
        self.guard.check(what)
        for k, v in {**self.fwd_out, **self.bwd_out, **self.g, "scratch": self.scratch}.items():
            assert bool((v == SENTINEL).all()), f"{what}: {k} was written"


@pytest.mark.parametrize("C", [64, 16])
def test_argument_checks(C):
    c = _Call(C)
    bad = dict(cin=0), dict(cin=9), dict(frames=0), dict(batch=-1), dict(video=None), dict(dims=None)
    for kw in bad:
        _refused(c.forward(**kw))
        _refused(c.backward(**kw))
        c.untouched(f"refused call {kw}")
    for ld in (999, 996, 0):
        _refused(c.forward(ctx_ld=ld))
        _refused(c.backward(dctx_ld=ld))
    _refused(c.forward(frames=2, ctx_ld=1024))
    _refused(c.backward(frames=2, dctx_ld=1024))
    for k in ("enc", "u1", "u2", "ctx"):
        _refused(c.forward(**{k: None}))
    for k in ("enc", "u1", "u2", "d_u2", "d_u1", "d_enc"):
        _refused(c.backward(**{k: None}))
    _refused(c.backward(dctx=None))
    c.untouched("refused calls (leading dimensions, NULL buffers)")
    # parameters and gradients: the forward reads all eight, the backward the up-sampler weights; all eight gradients
    for k in PNAMES:
        _refused(c.forward(vp=c.without("p", k)))
        _refused(c.backward(vg=c.without("g", k)))
    for k in ("up_w0", "up_w1", "up_w2"):
        _refused(c.backward(vp=c.without("p", k)))
    _refused(c.forward(vp=ctypes.POINTER(N.VideoParams)()))
    _refused(c.backward(vp=ctypes.POINTER(N.VideoParams)()))
    _refused(c.backward(vg=ctypes.POINTER(N.VideoParams)()))
    c.untouched("refused calls (NULL parameter / gradient)")
    # validate_dims' own code
    for d in (N.make_dims(2, 2, 64, 0, C), N.make_dims(0, 2, 64, C, C), N.make_dims(2, 2, 64, C, 0)):
        _refused(c.forward(dims=d), N.MVN_ERR_BAD_DIMS)
        _refused(c.backward(dims=d), N.MVN_ERR_BAD_DIMS)
    # an empty batch is no error and no work
    assert c.forward(batch=0) == N.MVN_OK and c.backward(batch=0) == N.MVN_OK
    c.untouched("batch = 0")
    # the calls these were variations of do run
    assert c.forward() == N.MVN_OK and c.backward() == N.MVN_OK
    c.guard.check("the valid calls")
    assert not bool((c.fwd_out["ctx"][:, :, :1000] == SENTINEL).any())
    assert bool((c.fwd_out["ctx"][:, :, 1000:] == SENTINEL).all())
    assert not bool((c.g["up_w2"] == SENTINEL).any())


def test_c64_backward_refuses_rows_it_cannot_load_16_bytes_at_a_time():
    """up_bwd64_kernel stages the rows of dctx / d_u2 / d_u1 with 16-byte loads: a leading dimension that is not a
    multiple of 4 floats, or a base that is not 16-byte aligned, is refused on the host (nothing is launched)"""
    c = _Call(64)
    for ld in (1001, 1002, 1003, 1022):
        _refused(c.backward(dctx_ld=ld))
    _refused(c.backward(dctx=c.dctx.data_ptr() + 4))
    _refused(c.backward(d_u2=c.bwd_out["d_u2"].data_ptr() + 8))
    _refused(c.backward(d_u1=c.bwd_out["d_u1"].data_ptr() + 4))
    c.untouched("refused calls (alignment)")
    assert c.backward(dctx_ld=1004) == N.MVN_OK
    c.guard.check("dctx_ld 1004")


# ---- 5. mvn_transpose_context ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("channels,t_len", [(16, 77), (24, 1000), (64, 33), (128, 2001), (64, 1), (24, 31)])
def test_transpose_context(B, channels, t_len):
    lib = N.lib()
    g = torch.Generator().manual_seed(channels + t_len)
    want = torch.randn(B, channels, t_len, generator=g)
    for ld in (t_len, t_len + 1, _wide(t_len)):
        guard = _Guard()
        ctx = guard.new((B, channels, ld), NAN, "ctx")   # NaN behind the valid columns
        ctx[:, :, :t_len] = want.to(DEV)
        out = guard.new((B, t_len, channels), SENTINEL, "context_tm")
        N.check(lib.mvn_transpose_context(ctx.data_ptr(), ld, B, channels, t_len, out.data_ptr(), _stream()),
                "mvn_transpose_context")
        guard.check("mvn_transpose_context")
        assert torch.equal(out.cpu(), want.permute(0, 2, 1)), (B, channels, t_len, ld)   # a pure copy


def test_transpose_context_argument_checks():
    lib = N.lib()
    guard = _Guard()
    ctx = guard.new((2, 16, 128), 1.0, "ctx")
    out = guard.new((2, 100, 16), SENTINEL, "context_tm")
    s = _stream()
    for args in ((None, 128, 2, 16, 100, out.data_ptr()), (ctx.data_ptr(), 128, 2, 16, 100, None),
                 (ctx.data_ptr(), 128, -1, 16, 100, out.data_ptr()), (ctx.data_ptr(), 128, 2, 0, 100, out.data_ptr()),
                 (ctx.data_ptr(), 128, 2, 16, 0, out.data_ptr()), (ctx.data_ptr(), 99, 2, 16, 100, out.data_ptr())):
        _refused(lib.mvn_transpose_context(*args, s))
    assert lib.mvn_transpose_context(ctx.data_ptr(), 128, 0, 16, 100, out.data_ptr(), s) == N.MVN_OK
    guard.check("mvn_transpose_context")
    assert bool((out == SENTINEL).all())
