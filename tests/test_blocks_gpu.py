"""GPU: the five building blocks (mvn_block_*, csrc/blocks.hip; movenet_amd.modules' forward methods) against
torch.nn.functional in float64 on the CPU, autograd for the gradients -- the expressions of oracle/wavenet_oracle.py's
causal_conv, gated_layer and dense_head.

Weights are scaled / sqrt(fan_in) so that activations and gradients are O(1); upstream gradients are seeded normal noise.
Bounds, as max |err| / max |ref| per tensor: forward 1e-5 (TOL_FWD of test_video_kernels_gpu.py), gradients 2e-5, widened
by helpers.grad_bound where the SAME reference computed in fp32 on the CPU is itself further than 5e-6 from float64.
Every case also checks that this fp32 CPU evaluation stays inside the bound the kernels are given.  No bound comes from
the kernels' own output.

Buffers handed to the C ABI are fronts of larger allocations with sentinel bands behind them (helpers._Guard), and with
ld > length the columns past the length are NaN: inputs that read one poison everything, outputs must leave them NaN.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from movenet_amd import _native as N
from movenet_amd import modules as M
from helpers import DEV, _Guard, grad_bound

pytestmark = pytest.mark.gpu

TOL_FWD = 1e-5


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _err(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert torch.isfinite(got).all(), "non-finite values in a result"
    return ((got - want).abs().max() / want.abs().max().clamp_min(1e-30)).item()


def _rng(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)


class Buf:
    """A (B, ch, len) tensor with row stride ld = len + pad inside a guarded allocation; columns past len are NaN."""

    def __init__(self, guard, shape, pad, src=None, name="buffer"):
        B, ch, n = shape
        self.full = guard.new((B, ch, n + pad), fill=float("nan"), name=name)
        self.view = self.full[:, :, :n]
        if src is not None:
            self.view.copy_(src.to(torch.float32))
        self.bt = N.BlockTensor(self.full.data_ptr(), n + pad, n)
        self.n, self.name = n, name

    def result(self):
        assert torch.isnan(self.full[:, :, self.n:]).all(), f"{self.name}: columns past the length were written"
        return self.view


def _check(case, fwd, grads, ref64, ref32):
    """fwd / grads: name -> device tensor; ref64 / ref32: name -> CPU tensor (float64 / the same in fp32)."""
    lines = []
    for name, got in {**fwd, **grads}.items():
        dev = _err(ref32[name], ref64[name])
        bound = TOL_FWD if name in fwd else grad_bound(dev)
        e = _err(got, ref64[name])
        lines.append(f"{name} {e:.2e}/{bound:.1e} (cpu fp32 {dev:.1e})")
        assert dev < bound, (case, name, "the fp32 CPU evaluation misses the bound", dev, bound)
        assert e < bound, (case, name, e, bound)
    print(f"{case}: " + " ".join(lines))


# ------------------------------------------------------------------------------------------------------------------
# gated layer through the C ABI
# ------------------------------------------------------------------------------------------------------------------
def _gated_case(Cc, K, d, n, B, s, ctx_len, seed=0):
    r = _rng(seed)
    T = n + d
    p = {"filter_w": r(Cc, Cc, 2) / math.sqrt(2 * Cc), "gate_w": r(Cc, Cc, 2) / math.sqrt(2 * Cc),
         "ctx_filter_w": r(Cc, Cc, 1) / math.sqrt(Cc), "ctx_filter_b": 0.5 * r(Cc),
         "ctx_gate_w": r(Cc, Cc, 1) / math.sqrt(Cc), "ctx_gate_b": 0.5 * r(Cc),
         "residual_w": r(Cc, Cc, 1) / math.sqrt(Cc), "residual_b": 0.5 * r(Cc),
         "skip_w": r(K, Cc, 1) / math.sqrt(Cc), "skip_b": 0.5 * r(K)}
    data = {"x": r(B, Cc, T), "ctx": r(B, Cc, ctx_len) if ctx_len else None, "d_res": r(B, Cc, n), "d_skip": r(B, K, s)}
    return p, data


def _gated_reference(p, data, d, s, dtype, use_res=True, use_skip=True):
    """oracle.gated_layer's expressions; returns forward values, saved activations and every gradient."""
    q = {k: v.to(dtype).clone().requires_grad_(True) for k, v in p.items()}
    x = data["x"].to(dtype).clone().requires_grad_(True)
    ctx = None if data["ctx"] is None else data["ctx"].to(dtype).clone().requires_grad_(True)
    f = F.conv1d(x, q["filter_w"], dilation=d)
    g = F.conv1d(x, q["gate_w"], dilation=d)
    if ctx is not None:
        c = ctx[:, :, -f.size(2):]
        f = f + F.conv1d(c, q["ctx_filter_w"], q["ctx_filter_b"])
        g = g + F.conv1d(c, q["ctx_gate_w"], q["ctx_gate_b"])
    th, sg = torch.tanh(f), torch.sigmoid(g)
    gated = th * sg
    res = F.conv1d(gated, q["residual_w"], q["residual_b"]) + x[:, :, -f.size(2):]
    skip = F.conv1d(gated, q["skip_w"], q["skip_b"])[:, :, -s:]
    loss = 0
    if use_res:
        loss = loss + (res * data["d_res"].to(dtype)).sum()
    if use_skip:
        loss = loss + (skip * data["d_skip"].to(dtype)).sum()
    loss.backward()
    out = {"residual": res, "skip": skip, "th": th, "sg": sg, "dx": x.grad}
    if ctx is not None:
        out["dctx"] = ctx.grad
    for k, v in q.items():
        if v.grad is not None:
            out["d_" + k] = v.grad
    return {k: v.detach() for k, v in out.items()}


def _pstruct(tensors):
    vals = []
    for k in N.BlockGatedParams._fields_:
        t = tensors.get(k[0])
        vals.append(None if t is None else t.data_ptr())
    return N.BlockGatedParams(*vals)


def _run_gated(Cc, K, d, n, B, s, ctx_len, pad, want_form, seed=0, null_dx=False, use_res=True, use_skip=True):
    """Forward and backward through the C ABI; returns (fwd, grads, raw gradient buffers) as device tensors."""
    lib = N.lib()
    p, data = _gated_case(Cc, K, d, n, B, s, ctx_len, seed)
    T = n + d
    guard = _Guard()
    pd = {k: guard.put(v.to(torch.float32).to(DEV), name=k) for k, v in p.items()}
    if not ctx_len:
        for k in ("ctx_filter_w", "ctx_filter_b", "ctx_gate_w", "ctx_gate_b"):
            pd.pop(k)
    x = Buf(guard, (B, Cc, T), pad, data["x"], "x")
    ctx = Buf(guard, (B, Cc, ctx_len), pad, data["ctx"], "ctx") if ctx_len else None
    res, skip = Buf(guard, (B, Cc, n), pad, name="residual"), Buf(guard, (B, K, s), pad, name="skip")
    th, sg = Buf(guard, (B, Cc, n), pad, name="th"), Buf(guard, (B, Cc, n), pad, name="sg")
    rc = lib.mvn_block_gated_forward(_pstruct(pd), Cc, K, d, x.bt, ctx.bt if ctx else None, res.bt, skip.bt, th.bt, sg.bt,
                                     B, None, 0, _stream())
    assert rc == 0, N.last_error()
    assert lib.mvn_block_last_form() == want_form
    fwd = {"residual": res.result(), "skip": skip.result(), "th": th.result(), "sg": sg.result()}

    # gradients accumulate: the buffers start from seeded non-zero values
    r = _rng(seed + 1000)
    g0 = {k: r(*v.shape).to(torch.float32).to(DEV) for k, v in pd.items()}
    gd = {k: guard.put(v, name="d_" + k) for k, v in g0.items()}
    d_res = Buf(guard, (B, Cc, n), pad, data["d_res"], "d_res") if use_res else None
    d_skip = Buf(guard, (B, K, s), pad, data["d_skip"], "d_skip") if use_skip else None
    dx = None if null_dx else Buf(guard, (B, Cc, T), pad, name="dx")
    dctx = Buf(guard, (B, Cc, ctx_len), pad, name="dctx") if (ctx and not null_dx) else None
    ns = lib.mvn_block_gated_scratch_floats(Cc, K, B, T, d, int(bool(ctx_len)), 1)
    scratch = guard.new((ns,), name="scratch")
    rc = lib.mvn_block_gated_backward(_pstruct(pd), _pstruct(gd), Cc, K, d, x.bt, ctx.bt if ctx else None, th.bt, sg.bt,
                                      d_res.bt if d_res else None, d_skip.bt if d_skip else None,
                                      dx.bt if dx else None, dctx.bt if dctx else None, B, scratch.data_ptr(), ns, _stream())
    assert rc == 0, N.last_error()
    assert lib.mvn_block_last_form() == N.BLOCK_FORM_GENERIC  # the backward is composed from the generic family
    guard.check(f"gated C={Cc} K={K} d={d} n={n}")
    grads = {"d_" + k: (gd[k].double() - g0[k].double()).reshape(p[k].shape) for k in gd}
    if not use_res:
        assert torch.equal(gd["residual_w"], g0["residual_w"]) and torch.equal(gd["residual_b"], g0["residual_b"])
        grads.pop("d_residual_w"), grads.pop("d_residual_b")
    if dx:
        grads["dx"] = dx.result()
    if dctx:
        grads["dctx"] = dctx.result()
    return fwd, grads, gd, (p, data)


def _gated_checked(Cc, K, d, n, B, s, ctx_len, pad, want_form, **kw):
    case = f"gated C={Cc} K={K} d={d} n={n} B={B} s={s} ctx={ctx_len} pad={pad} {kw}"
    fwd, grads, raw, (p, data) = _run_gated(Cc, K, d, n, B, s, ctx_len, pad, want_form, **kw)
    rk = {k: kw[k] for k in ("use_res", "use_skip") if k in kw}
    ref64 = _gated_reference(p, data, d, s, torch.float64, **rk)
    ref32 = _gated_reference(p, data, d, s, torch.float32, **rk)
    if not kw.get("use_skip", True):
        grads.pop("d_skip_w"), grads.pop("d_skip_b")
    _check(case, fwd, grads, ref64, ref32)
    return raw


@pytest.mark.parametrize("d", [1, 2, 512])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_gated_fused_form(d, n):
    """C = K = 64: the fused forward kernel (form 2), backward from the generic family.  Per (d, T - d): no context,
    Tc == T - d and Tc == T; B, skip_size and the row stride cycle so that every listed value meets every d and length."""
    i = [1, 2, 512].index(d) + [1, 63, 64, 65, 200].index(n)
    for j, ctx_len in enumerate((0, n, n + d)):
        B = (1, 3)[(i + j) % 2]
        s = (1, min(37, n), n)[(i + j) % 3]
        pad = (0, 5)[(i + j // 2) % 2]
        _gated_checked(64, 64, d, n, B, s, ctx_len, pad, N.BLOCK_FORM_FUSED64, seed=10 * i + j)


def test_gated_fused_every_skip_size_and_stride():
    for n, d in ((65, 1), (200, 2), (63, 512)):
        for s in (1, 37, n):
            for pad in (0, 5):
                _gated_checked(64, 64, d, n, 3, s, n + d, pad, N.BLOCK_FORM_FUSED64, seed=s + pad)


def test_gated_null_gradients_and_unused_outputs():
    # dx / dcontext NULL: the parameter gradients are still complete
    _gated_checked(64, 64, 2, 65, 3, 37, 67, 5, N.BLOCK_FORM_FUSED64, null_dx=True)
    # an output that received no gradient
    _gated_checked(64, 64, 2, 65, 1, 37, 65, 0, N.BLOCK_FORM_FUSED64, use_res=False)
    _gated_checked(64, 64, 1, 200, 3, 37, 0, 5, N.BLOCK_FORM_FUSED64, use_skip=False)
    _gated_checked(24, 40, 4, 65, 1, 9, 65, 0, N.BLOCK_FORM_GENERIC, use_res=False)


def test_gated_two_runs_bit_equal():
    for Cc, K, n, form in ((64, 64, 200, N.BLOCK_FORM_FUSED64), (24, 40, 65, N.BLOCK_FORM_GENERIC)):
        a = _run_gated(Cc, K, 2, n, 3, 37, n + 2, 5, form, seed=3)
        b = _run_gated(Cc, K, 2, n, 3, 37, n + 2, 5, form, seed=3)
        for k in a[0]:
            assert torch.equal(a[0][k], b[0][k]), k
        for k in a[2]:
            assert torch.equal(a[2][k], b[2][k]), k
        assert torch.equal(a[1]["dx"], b[1]["dx"]) and torch.equal(a[1]["dctx"], b[1]["dctx"])


@pytest.mark.parametrize("Cc,K", [(8, 4), (16, 8), (24, 40), (128, 128), (256, 256)])
def test_gated_generic_form(Cc, K):
    i = 0
    for d in (1, 4):
        for n in (1, 65):
            for ctx_len in (0, n + d):
                s = (1, n)[i % 2] if n == 1 else (1, 37, n)[i % 3]
                _gated_checked(Cc, K, d, n, (1, 3)[i % 2], s, ctx_len, (0, 5)[(i // 2) % 2], N.BLOCK_FORM_GENERIC, seed=i)
                i += 1


# ------------------------------------------------------------------------------------------------------------------
# the two-tap convolutions and the head through the C ABI
# ------------------------------------------------------------------------------------------------------------------
def _conv_reference(w, b, x, dy, dilation, dtype):
    w, x = w.to(dtype).clone().requires_grad_(True), x.to(dtype).clone().requires_grad_(True)
    b = None if b is None else b.to(dtype).clone().requires_grad_(True)
    if dilation == 0:
        y = F.conv1d(x, w, b, padding=1)[:, :, :-1]
    else:
        y = F.conv1d(x, w, b, dilation=dilation)
    (y * dy.to(dtype)).sum().backward()
    out = {"y": y, "dx": x.grad, "dw": w.grad}
    if b is not None:
        out["db"] = b.grad
    return {k: v.detach() for k, v in out.items()}


def _conv_checked(cin, cout, T, dilation, bias, B, pad, seed):
    lib = N.lib()
    r = _rng(seed)
    n = T - dilation
    w, b = r(cout, cin, 2) / math.sqrt(2 * cin), (0.5 * r(cout) if bias else None)
    xs, dys = r(B, cin, T), r(B, cout, n)
    guard = _Guard()
    wd = guard.put(w.float().to(DEV), "w")
    bd = guard.put(b.float().to(DEV), "b") if bias else None
    x, y = Buf(guard, (B, cin, T), pad, xs, "x"), Buf(guard, (B, cout, n), pad, name="y")
    dy, dx = Buf(guard, (B, cout, n), pad, dys, "dy"), Buf(guard, (B, cin, T), pad, name="dx")
    g0w, g0b = r(cout, cin, 2).float().to(DEV), r(cout).float().to(DEV)
    dw, db = guard.put(g0w, "dw"), (guard.put(g0b, "db") if bias else None)
    ns = lib.mvn_block_conv_scratch_floats(cin, cout, B, n)
    scratch = guard.new((ns,), name="scratch")
    bp, dbp = (bd.data_ptr() if bias else None), (db.data_ptr() if bias else None)
    if dilation == 0:
        rc = lib.mvn_block_causal_forward(wd.data_ptr(), bp, cin, cout, x.bt, y.bt, B, _stream())
        assert rc == 0, N.last_error()
        rc = lib.mvn_block_causal_backward(wd.data_ptr(), cin, cout, x.bt, dy.bt, dx.bt, dw.data_ptr(), dbp, B,
                                           scratch.data_ptr(), ns, _stream())
    else:
        rc = lib.mvn_block_dilated_forward(wd.data_ptr(), bp, cin, dilation, x.bt, y.bt, B, _stream())
        assert rc == 0, N.last_error()
        rc = lib.mvn_block_dilated_backward(wd.data_ptr(), cin, dilation, x.bt, dy.bt, dx.bt, dw.data_ptr(), dbp, B,
                                            scratch.data_ptr(), ns, _stream())
    assert rc == 0, N.last_error()
    assert lib.mvn_block_last_form() == N.BLOCK_FORM_GENERIC
    case = f"conv {cin}->{cout} T={T} d={dilation} bias={bias} B={B} pad={pad}"
    guard.check(case)
    ref64 = _conv_reference(w, b, xs, dys, dilation, torch.float64)
    ref32 = _conv_reference(w, b, xs, dys, dilation, torch.float32)
    grads = {"dx": dx.result(), "dw": dw.double() - g0w.double()}
    if bias:
        grads["db"] = db.double() - g0b.double()
    yv = y.result()
    _check(case, {"y": yv}, grads, ref64, ref32)
    if dilation == 0:  # column 0 sees the left padding: only the second tap
        col0 = torch.einsum("oi,bi->bo", w[:, :, 1], xs[:, :, 0]) + (b if bias else 0)
        assert _err(yv[:, :, 0], col0) < TOL_FWD


@pytest.mark.parametrize("cin,cout", [(16, 8), (256, 64)])
@pytest.mark.parametrize("bias", [False, True])
def test_causal_conv(cin, cout, bias):
    for i, T in enumerate((1, 2, 65)):
        _conv_checked(cin, cout, T, 0, bias, (1, 3)[i % 2], (0, 5)[i % 2], seed=i)


@pytest.mark.parametrize("channels", [8, 64])
def test_dilated_conv(channels):
    i = 0
    for d in (1, 8):
        for n in (1, 65):
            _conv_checked(channels, channels, n + d, d, bool(i % 2), (3, 1)[i % 2], (5, 0)[i % 2], seed=20 + i)
            i += 1


def _dense_reference(p, x, dy, dtype):
    q = {k: v.to(dtype).clone().requires_grad_(True) for k, v in p.items()}
    x = x.to(dtype).clone().requires_grad_(True)
    h = F.conv1d(F.leaky_relu(x), q["w1"], q["b1"])
    y = F.conv1d(F.leaky_relu(h), q["w2"], q["b2"])
    (y * dy.to(dtype)).sum().backward()
    out = {"y": y, "h": h, "dx": x.grad, **{"d" + k: v.grad for k, v in q.items()}}
    return {k: v.detach() for k, v in out.items()}


@pytest.mark.parametrize("K,Q", [(64, 256), (64, 128), (4, 32)])
def test_dense_head(K, Q):
    lib = N.lib()
    for i, S in enumerate((1, 65, 130)):
        B, pad = (1, 3)[i % 2], (0, 5)[i % 2]
        r = _rng(40 + i)
        p = {"w1": r(Q, K, 1) / math.sqrt(K), "b1": 0.5 * r(Q), "w2": r(Q, Q, 1) / math.sqrt(Q), "b2": 0.5 * r(Q)}
        xs, dys = r(B, K, S) - 0.3, r(B, Q, S)  # both signs: both slopes of the leaky ReLUs
        assert (xs < 0).any() and (xs > 0).any()
        guard = _Guard()
        pd = {k: guard.put(v.float().to(DEV), k) for k, v in p.items()}
        g0 = {k: r(*v.shape).float().to(DEV) for k, v in p.items()}
        gd = {k: guard.put(v, "d" + k) for k, v in g0.items()}
        x, h, y = Buf(guard, (B, K, S), pad, xs, "x"), Buf(guard, (B, Q, S), pad, name="h"), Buf(guard, (B, Q, S), pad, name="y")
        dy, dx = Buf(guard, (B, Q, S), pad, dys, "dy"), Buf(guard, (B, K, S), pad, name="dx")
        rc = lib.mvn_block_dense_forward(pd["w1"].data_ptr(), pd["b1"].data_ptr(), pd["w2"].data_ptr(), pd["b2"].data_ptr(),
                                         K, Q, x.bt, h.bt, y.bt, B, None, 0, _stream())
        assert rc == 0, N.last_error()
        # ... and without a hidden buffer the same output comes from the scratch
        y2 = Buf(guard, (B, Q, S), pad, name="y2")
        nf = lib.mvn_block_dense_scratch_floats(K, Q, B, S, 0)
        sf = guard.new((nf,), name="scratch fwd")
        rc = lib.mvn_block_dense_forward(pd["w1"].data_ptr(), pd["b1"].data_ptr(), pd["w2"].data_ptr(), pd["b2"].data_ptr(),
                                         K, Q, x.bt, None, y2.bt, B, sf.data_ptr(), nf, _stream())
        assert rc == 0, N.last_error()
        ns = lib.mvn_block_dense_scratch_floats(K, Q, B, S, 1)
        scratch = guard.new((ns,), name="scratch")
        rc = lib.mvn_block_dense_backward(pd["w1"].data_ptr(), pd["w2"].data_ptr(), K, Q, x.bt, h.bt, dy.bt, dx.bt,
                                          gd["w1"].data_ptr(), gd["b1"].data_ptr(), gd["w2"].data_ptr(), gd["b2"].data_ptr(),
                                          B, scratch.data_ptr(), ns, _stream())
        assert rc == 0, N.last_error()
        case = f"dense {K}->{Q} S={S} B={B} pad={pad}"
        guard.check(case)
        assert torch.equal(y.result(), y2.result())
        ref64, ref32 = _dense_reference(p, xs, dys, torch.float64), _dense_reference(p, xs, dys, torch.float32)
        assert (ref64["h"] < 0).any() and (ref64["h"] > 0).any()
        grads = {"dx": dx.result(), **{"d" + k: gd[k].double() - g0[k].double() for k in gd}}
        _check(case, {"y": y.result(), "h": h.result()}, grads, ref64, ref32)


# ------------------------------------------------------------------------------------------------------------------
# modules and autograd
# ------------------------------------------------------------------------------------------------------------------
def _scaled(module, seed):
    """Seeded parameters / sqrt(fan_in) (biases 0.5 N(0, 1)), as float64 CPU tensors; the module gets their fp32 copy."""
    r = _rng(seed)
    vals = {}
    with torch.no_grad():
        for name, q in module.named_parameters():
            v = r(*q.shape) / math.sqrt(q.shape[1] * q.shape[2]) if q.dim() == 3 else 0.5 * r(*q.shape)
            vals[name] = v
            q.copy_(v.to(torch.float32))
    return vals


def _stack_reference(vals, dilations, x, ctx, s, up, dtype):
    """torch.stack of the float64 chain of oracle.gated_layer's expressions (movenet/modules.py:119-130)."""
    q = {k: v.to(dtype).clone().requires_grad_(True) for k, v in vals.items()}
    x = x.to(dtype).clone().requires_grad_(True)
    ctx = None if ctx is None else ctx.to(dtype).clone().requires_grad_(True)
    h, skips = x, []
    for l, d in enumerate(dilations):
        pre = f"conv_layers.{l}."
        f = F.conv1d(h, q[pre + "conv_filter.conv.weight"], dilation=d)
        g = F.conv1d(h, q[pre + "conv_gate.conv.weight"], dilation=d)
        if ctx is not None:
            c = ctx[:, :, -f.size(2):]
            f = f + F.conv1d(c, q[pre + "context_conv_filter.weight"], q[pre + "context_conv_filter.bias"])
            g = g + F.conv1d(c, q[pre + "context_conv_gate.weight"], q[pre + "context_conv_gate.bias"])
        gated = torch.tanh(f) * torch.sigmoid(g)
        res = F.conv1d(gated, q[pre + "conv_residual.weight"], q[pre + "conv_residual.bias"]) + h[:, :, -f.size(2):]
        skips.append(F.conv1d(gated, q[pre + "conv_skip.weight"], q[pre + "conv_skip.bias"])[:, :, -s:])
        h = res
    out = torch.stack(skips)
    (out * up.to(dtype)).sum().backward()
    ref = {"out": out.detach(), "dx": x.grad}
    if ctx is not None:
        ref["dctx"] = ctx.grad
    for k, v in q.items():
        ref[k] = v.grad  # None where the parameter does not reach the output
    return ref


@pytest.mark.parametrize("Cc,K", [(64, 64), (8, 4)])
@pytest.mark.parametrize("with_ctx", [False, True])
def test_residual_stack_module(Cc, K, with_ctx):
    B, T = 2, 40
    stack = M.ResidualConvStack(3, 2, Cc, K).to(DEV)
    vals = _scaled(stack, 5)
    r = _rng(6)
    for s in (1, 26):
        xs, cs = r(B, Cc, T), (r(B, Cc, T) if with_ctx else None)
        up = r(6, B, K, s)
        x = xs.float().to(DEV).requires_grad_(True)
        ctx = cs.float().to(DEV).requires_grad_(True) if with_ctx else None
        stack.zero_grad(set_to_none=True)
        out = stack(x, ctx, s)
        assert out.shape == (6, B, K, s)
        assert N.lib().mvn_block_last_form() == (N.BLOCK_FORM_FUSED64 if Cc == 64 else N.BLOCK_FORM_GENERIC)
        (out * up.float().to(DEV)).sum().backward()
        ref64 = _stack_reference(vals, stack.dilations, xs, cs, s, up, torch.float64)
        ref32 = _stack_reference(vals, stack.dilations, xs, cs, s, up, torch.float32)
        grads = {"dx": x.grad}
        if with_ctx:
            grads["dctx"] = ctx.grad
        for name, q in stack.named_parameters():
            if ref64[name] is None:  # the last layer's conv_residual, and the context convs without a context
                assert q.grad is None, name
            else:
                assert q.grad is not None, name
                grads[name] = q.grad
        ref64 = {k: v for k, v in ref64.items() if v is not None}
        ref32 = {k: v for k, v in ref32.items() if v is not None}
        assert ref64["conv_layers.5.conv_skip.weight"] is not None and "conv_layers.5.conv_residual.weight" not in ref64
        _check(f"stack C={Cc} K={K} ctx={with_ctx} s={s}", {"out": out}, grads, ref64, ref32)


def test_value_errors_of_the_modules():
    layer = M.GatedResidualConv1d(8, 4, 2).to(DEV)
    x = torch.randn(1, 8, 10, device=DEV)
    with pytest.raises(ValueError, match="negative"):
        layer(x, None, -1)
    with pytest.raises(ValueError, match="context"):
        layer(x, torch.randn(1, 8, 7, device=DEV), 3)
    with pytest.raises(RuntimeError, match="T = 2.*d = 2"):
        layer(x[:, :, :2], None, 1)
    with pytest.raises(RuntimeError, match="T = 2.*d = 2"):
        M.DilatedCausalConv1d(8, dilation=2).to(DEV)(x[:, :, :2])
    # Python slicing: 0 and values above T - d return all T - d columns
    assert layer(x, None, 0)[1].shape == (1, 4, 8) and layer(x, None, 99)[1].shape == (1, 4, 8)
    assert layer(x, None, 3)[1].shape == (1, 4, 3) and layer(x, None, 3)[0].shape == (1, 8, 8)
    stack = M.ResidualConvStack(3, 2, 8, 4).to(DEV)
    x = torch.randn(1, 8, 40, device=DEV)
    for s in (0, -1, 27):
        with pytest.raises(ValueError, match="skip_size"):
            stack(x, None, s)
    with pytest.raises(ValueError, match="aligned"):
        stack(x, torch.randn(1, 8, 39, device=DEV), 5)
    with pytest.raises(RuntimeError, match="holds parameters"):
        stack(x.cpu(), None, 5)


def test_composition_equals_the_model():
    """dense_conv(stack(causal_conv(x), None, S).sum(0)) and WaveNet.forward on the same weights: each within the
    forward bound of float64 (not bit-equal: the products run in different forms).  Gradients: the model differentiates
    with respect to its parameters only (its input enters as indices), so the parameter gradients of both paths are held
    against float64, and the block path's input gradient as well."""
    import movenet_amd.wavenet as W
    m = W.WaveNet(3, 2, 64, residual_channels=64, skip_channels=64).to(DEV)
    vals = {k: v for k, v in _scaled(m, 7).items()}
    B, T = 2, 40
    S = m.compute_output_size(torch.empty(B, 64, T))  # the model's own skip_size with remove_last=False
    idx = torch.randint(0, 64, (B, T), generator=torch.Generator().manual_seed(9))
    xs = F.one_hot(idx, 64).permute(0, 2, 1).double()
    up = _rng(8)(B, 64, S)
    used = [k for k in vals if k.split(".")[0] in ("causal_conv", "residual_conv_stack", "dense_conv")
            and "context_conv" not in k]

    def reference(dtype):
        q = {k: vals[k].to(dtype).clone().requires_grad_(True) for k in used}
        x = xs.to(dtype).clone().requires_grad_(True)
        h = F.conv1d(x, q["causal_conv.conv.weight"], padding=1)[:, :, :-1]
        skips = []
        for l, d in enumerate(m.residual_conv_stack.dilations):
            pre = f"residual_conv_stack.conv_layers.{l}."
            f = F.conv1d(h, q[pre + "conv_filter.conv.weight"], dilation=d)
            g = F.conv1d(h, q[pre + "conv_gate.conv.weight"], dilation=d)
            gated = torch.tanh(f) * torch.sigmoid(g)
            res = F.conv1d(gated, q[pre + "conv_residual.weight"], q[pre + "conv_residual.bias"]) + h[:, :, -f.size(2):]
            skips.append(F.conv1d(gated, q[pre + "conv_skip.weight"], q[pre + "conv_skip.bias"])[:, :, -S:])
            h = res
        y = F.conv1d(F.leaky_relu(torch.stack(skips).sum(0)), q["dense_conv.conv1.weight"], q["dense_conv.conv1.bias"])
        y = F.conv1d(F.leaky_relu(y), q["dense_conv.conv2.weight"], q["dense_conv.conv2.bias"])
        (y * up.to(dtype)).sum().backward()
        out = {"y": y.detach(), "dx": x.grad}
        out.update({k: v.grad for k, v in q.items() if v.grad is not None})
        return out

    ref64, ref32 = reference(torch.float64), reference(torch.float32)
    params = dict(m.named_parameters())
    reach = [k for k in used if k in ref64]
    assert "residual_conv_stack.conv_layers.5.conv_residual.weight" not in reach and len(reach) == len(used) - 2

    x1 = xs.float().to(DEV).requires_grad_(True)
    y1 = m.dense_conv(m.residual_conv_stack(m.causal_conv(x1), None, S).sum(0))
    (y1 * up.float().to(DEV)).sum().backward()
    grads = {k: params[k].grad.clone() for k in reach}
    grads["dx"] = x1.grad
    _check("composition: blocks", {"y": y1}, grads, ref64, ref32)

    m.zero_grad(set_to_none=True)
    y2 = m(xs.float().to(DEV), output_unnormalized=False, remove_last=False)
    assert y2.shape == y1.shape
    (y2 * up.float().to(DEV)).sum().backward()
    _check("composition: model", {"y": y2}, {k: params[k].grad for k in reach}, ref64, ref32)


def test_block_inside_another_graph():
    layer = M.GatedResidualConv1d(64, 64, 2).to(DEV)
    vals = _scaled(layer, 11)
    xs = _rng(12)(3, 64, 30)
    x = xs.float().to(DEV).requires_grad_(True)
    torch.tanh(layer(x, None, 5)[1]).sum().backward()
    assert N.lib().mvn_block_last_form() == N.BLOCK_FORM_GENERIC  # (the backward ran last)

    def reference(dtype):
        q = {k: v.to(dtype) for k, v in vals.items()}
        xr = xs.to(dtype).clone().requires_grad_(True)
        f = F.conv1d(xr, q["conv_filter.conv.weight"], dilation=2)
        g = F.conv1d(xr, q["conv_gate.conv.weight"], dilation=2)
        skip = F.conv1d(torch.tanh(f) * torch.sigmoid(g), q["conv_skip.weight"], q["conv_skip.bias"])[:, :, -5:]
        torch.tanh(skip).sum().backward()
        return {"dx": xr.grad}

    _check("gated layer under tanh().sum()", {}, {"dx": x.grad}, reference(torch.float64), reference(torch.float32))
    assert layer.conv_residual.weight.grad is None and layer.conv_skip.weight.grad is not None
