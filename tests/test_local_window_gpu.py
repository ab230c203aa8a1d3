"""GPU: mvn_upsample_features_win and its backward through the C ABI, on guarded buffers, against float64
(tests/local_window_reference: replicate padding + conv1d + the interpolation expression, gradients by autograd).

Bounds: those of tests/test_upsample_features_gpu.py -- forward max |err| / max |ref| below 1e-5 (its TOL_FWD), gradients
below helpers.grad_bound of the deviation the same expression shows in fp32 on the CPU; the two edge frames of dmel are
also held to that bound on their own, relative to their own maximum, so an edge error is not averaged away.  Everything
else is bit equality: two calls, a row stride above the row length with NaN behind the rows, taps = 1 against the
existing entry points, the Python op against the C calls.  Measured: DESIGN 4.5h."""
import functools

import pytest
import torch

import local_window_reference as W
from helpers import DEV, SENTINEL, _Guard, grad_bound
from movenet_amd import _native as N

pytestmark = pytest.mark.gpu
TOL_FWD = 1e-5
# (B, M, F, C, hop, T, k)
PLAIN, PLAIN_ON_FRAME = (2, 5, 7, 16, 16, 100, 1), (2, 5, 7, 16, 16, 97, 2)   # 97 - 1 = 6 x 16: T - 1 on a frame
ALL_CLAMP_1, ALL_CLAMP_3 = (1, 4, 1, 4, 16, 16, 2), (2, 3, 3, 8, 4, 9, 4)     # F <= k: every tap of every frame clamps
MULTI = (2, 5, 71, 16, 16, 1101, 2)     # frames 63 | 64 sit in two workgroups of the projection and of dmel and take
#                                         their neighbours across that boundary; 69 frames needed of 71: a surplus frame
WIDE = (1, 4, 65, 4, 16, 1024, 8)       # taps = 17 against a second workgroup of ONE frame
WORKLOAD = (1, 80, 5, 64, 256, 1000, 2)  # the workload's own M, C and hop at five frames
SHAPES = [PLAIN, PLAIN_ON_FRAME, ALL_CLAMP_1, ALL_CLAMP_3, MULTI, WIDE, WORKLOAD]


def _err(got, want):
    return ((got.double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-30)).item()


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _with_edges(r):
    """A reference's tensors, and the two edge frames of dmel as entries of their own."""
    return {**r, "dmel_first": r["dmel"][:, :, 0], "dmel_last": r["dmel"][:, :, -1]}


@functools.lru_cache(maxsize=None)
def _case(shape):
    B, M, F, C, hop, T, k = shape
    taps = 2 * k + 1
    g = torch.Generator().manual_seed(sum(p * v for p, v in zip((7, 11, 13, 17, 19, 23, 29), shape)))
    mel, w = torch.randn(B, M, F, generator=g), torch.randn(C, M, taps, generator=g) / (M * taps) ** 0.5
    bias, dctx = torch.randn(C, generator=g), torch.randn(B, C, T, generator=g)
    g0 = dict(dw=torch.randn(C, M, taps, generator=g), dbias=torch.randn(C, generator=g))  # what the buffers hold before
    ref = _with_edges(W.reference(mel, w, bias, dctx, hop, T, torch.float64))
    ref32 = _with_edges(W.reference(mel, w, bias, dctx, hop, T, torch.float32))
    return mel, w, bias, dctx, g0, ref, {key: _err(ref32[key], ref[key]) for key in ref}


def _padded(guard, t, pad, name):
    """``t`` (B, R, L) as the first L columns of the rows of a (B, R, L + pad) buffer whose other columns hold NaN."""
    if pad == 0:
        return guard.put(t, name)
    buf = guard.new((t.shape[0], t.shape[1], t.shape[2] + pad), float("nan"), name)
    buf[:, :, :t.shape[2]].copy_(t)
    return buf


def _run_forward(guard, mel, w, bias, hop, T, ctx_ld=None, mel_pad=0, taps=None, frames=None, scratch_floats=None):
    """rc and the (B, C, ctx_ld) output; ``taps`` / ``frames`` / ``scratch_floats`` override what the tensors say."""
    lib = N.lib()
    (B, M, F), C = mel.shape, w.shape[0]
    ctx_ld = (T + 3) // 4 * 4 if ctx_ld is None else ctx_ld
    mel_d, w_d, bias_d = _padded(guard, mel, mel_pad, "mel"), guard.put(w, "w"), guard.put(bias, "bias")
    ctx = guard.new((B, C, ctx_ld), SENTINEL, "ctx")
    n = lib.mvn_upsample_features_scratch_floats(B, C, F)
    scratch = guard.new((n,), SENTINEL, "scratch")
    rc = lib.mvn_upsample_features_win(mel_d.data_ptr(), F + mel_pad, w_d.data_ptr(), bias_d.data_ptr(), B, M,
                                       F if frames is None else frames, C, w.shape[2] if taps is None else taps, hop, T,
                                       ctx.data_ptr(), ctx_ld, scratch.data_ptr(),
                                       n if scratch_floats is None else scratch_floats, _stream())
    return rc, ctx, scratch


def _run_backward(guard, mel, w, dctx, g0, hop, T, want=("dw", "dbias", "dmel"), mel_pad=0, dmel_pad=0):
    """dict(dw, dbias, dmel) on the device (None where not wanted: NULL was passed), dw and dbias accumulated into
    ``g0``'s values."""
    lib = N.lib()
    (B, M, F), C, taps = mel.shape, w.shape[0], w.shape[2]
    mel_d, w_d, dctx_d = _padded(guard, mel, mel_pad, "mel"), guard.put(w, "w"), guard.put(dctx, "dctx")
    out = dict(dw=guard.put(g0["dw"], "dw") if "dw" in want else None,
               dbias=guard.put(g0["dbias"], "dbias") if "dbias" in want else None,
               dmel=guard.new((B, M, F + dmel_pad), SENTINEL, "dmel") if "dmel" in want else None)
    n = lib.mvn_upsample_features_scratch_floats(B, C, F)
    scratch = guard.new((n,), float("nan"), "scratch")
    ptr = {key: (v.data_ptr() if v is not None else None) for key, v in out.items()}
    N.check(lib.mvn_upsample_features_win_backward(dctx_d.data_ptr(), T, mel_d.data_ptr(), F + mel_pad, w_d.data_ptr(), B,
                                                   M, F, C, taps, hop, T, ptr["dw"], ptr["dbias"], ptr["dmel"],
                                                   F + dmel_pad, scratch.data_ptr(), n, _stream()),
            "mvn_upsample_features_win_backward")
    guard.check("mvn_upsample_features_win_backward")
    return out


@functools.lru_cache(maxsize=None)
def _contiguous(shape, zero_start=False):
    """The contiguous C calls on ``shape``, on the CPU: (ctx[:, :, :T], dw, dbias, dmel); ``zero_start``: dw and dbias
    accumulated into zeros, as ops.upsample_features does."""
    hop, T = shape[4], shape[5]
    mel, w, bias, dctx, g0 = _case(shape)[:5]
    guard = _Guard()
    rc, ctx, _ = _run_forward(guard, mel, w, bias, hop, T)
    N.check(rc, "mvn_upsample_features_win")
    guard.check("mvn_upsample_features_win")
    start = {key: torch.zeros_like(v) for key, v in g0.items()} if zero_start else g0
    got = _run_backward(guard, mel, w, dctx, start, hop, T)
    return ctx[:, :, :T].cpu(), got["dw"].cpu(), got["dbias"].cpu(), got["dmel"].cpu()


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_against_float64(shape):
    B, M, F, C, hop, T, k = shape
    mel, w, bias = _case(shape)[:3]
    ref = _case(shape)[5]
    guard = _Guard()
    ld = (T + 3) // 4 * 4 + 8
    rc, ctx, _ = _run_forward(guard, mel, w, bias, hop, T, ctx_ld=ld)
    N.check(rc, "mvn_upsample_features_win")
    guard.check("mvn_upsample_features_win")
    assert bool((ctx[:, :, T:] == SENTINEL).all()), "columns past T were written"
    e = _err(ctx[:, :, :T], ref["ctx"])
    print(f"upsample_features_win forward {shape}: {e:.2e}")
    assert e < TOL_FWD, (shape, e)
    # two calls: the same bits
    assert torch.equal(ctx[:, :, :T].cpu(), _contiguous(shape)[0])


@pytest.mark.parametrize("shape", SHAPES)
def test_backward_against_float64_autograd(shape):
    B, M, F, C, hop, T, k = shape
    mel, w, _, dctx, g0, ref, dev = _case(shape)
    full = _run_backward(_Guard(), mel, w, dctx, g0, hop, T)
    # dw and dbias were accumulated INTO the random values the buffers held
    got = dict(dw=full["dw"].cpu() - g0["dw"], dbias=full["dbias"].cpu() - g0["dbias"], dmel=full["dmel"].cpu())
    got.update(dmel_first=got["dmel"][:, :, 0], dmel_last=got["dmel"][:, :, -1])
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    worst = {key: _err(got[key], ref[key]) for key in got}
    print(f"upsample_features_win backward {shape}: "
          + " ".join(f"{key} {v:.2e}/{grad_bound(dev[key]):.1e}" for key, v in worst.items()))
    for key, e in worst.items():
        assert e < grad_bound(dev[key]), (shape, key, e, dev[key])
    # two calls: the same bits
    _, dw0, db0, dmel0 = _contiguous(shape)
    assert torch.equal(full["dw"].cpu(), dw0) and torch.equal(full["dbias"].cpu(), db0)
    assert torch.equal(full["dmel"].cpu(), dmel0)
    # each of the three as NULL: the other two are the same bits again
    for absent in ("dw", "dbias", "dmel"):
        rest = tuple(key for key in ("dw", "dbias", "dmel") if key != absent)
        part = _run_backward(_Guard(), mel, w, dctx, g0, hop, T, want=rest)
        assert part[absent] is None
        for key in rest:
            assert torch.equal(part[key], full[key]), (shape, absent, key)


@pytest.mark.parametrize("shape", [MULTI, ALL_CLAMP_3])
def test_nan_behind_the_mel_rows_is_never_read(shape):
    """mel_ld = F + 3, the three columns behind every row NaN (and dmel_ld = F + 3): the bits of the contiguous calls --
    the clamp stops at the last frame GIVEN, and nothing at or beyond column F is read or written."""
    B, M, F, C, hop, T, k = shape
    mel, w, bias, dctx, g0 = _case(shape)[:5]
    ctx0, dw0, db0, dmel0 = _contiguous(shape)
    guard = _Guard()
    rc, ctx, _ = _run_forward(guard, mel, w, bias, hop, T, mel_pad=3)
    N.check(rc, "mvn_upsample_features_win")
    guard.check("mvn_upsample_features_win (mel_ld = F + 3)")
    assert bool(torch.isfinite(ctx[:, :, :T]).all()) and torch.equal(ctx[:, :, :T].cpu(), ctx0)
    got = _run_backward(guard, mel, w, dctx, g0, hop, T, mel_pad=3, dmel_pad=3)
    assert all(bool(torch.isfinite(got[key]).all()) for key in ("dw", "dbias"))
    assert torch.equal(got["dw"].cpu(), dw0) and torch.equal(got["dbias"].cpu(), db0)
    assert torch.equal(got["dmel"][:, :, :F].cpu(), dmel0)
    assert bool((got["dmel"][:, :, F:] == SENTINEL).all()), "padding columns of dmel were written"


@pytest.mark.parametrize("shape", [MULTI, PLAIN_ON_FRAME])
def test_one_tap_gives_the_bits_of_the_existing_entry_points(shape):
    B, M, F, C, hop, T, _ = shape
    mel, w, bias, dctx, g0 = _case(shape)[:5]
    w1 = w[:, :, :1].contiguous()
    g1 = dict(dw=g0["dw"][:, :, :1].contiguous(), dbias=g0["dbias"])
    lib = N.lib()
    guard = _Guard()
    rc, ctx, _ = _run_forward(guard, mel, w1, bias, hop, T)
    N.check(rc, "mvn_upsample_features_win")
    got = _run_backward(guard, mel, w1, dctx, g1, hop, T)
    # the existing calls, on the same values
    mel_d, w_d, bias_d, dctx_d = (guard.put(v, "old") for v in (mel, w1[:, :, 0].contiguous(), bias, dctx))
    ld = (T + 3) // 4 * 4
    old = guard.new((B, C, ld), SENTINEL, "ctx")
    dw, db = guard.put(g1["dw"][:, :, 0].contiguous(), "dw"), guard.put(g1["dbias"], "dbias")
    dmel = guard.new((B, M, F), SENTINEL, "dmel")
    n = lib.mvn_upsample_features_scratch_floats(B, C, F)
    scratch = guard.new((n,), float("nan"), "scratch")
    N.check(lib.mvn_upsample_features(mel_d.data_ptr(), F, w_d.data_ptr(), bias_d.data_ptr(), B, M, F, C, hop, T,
                                      old.data_ptr(), ld, scratch.data_ptr(), n, _stream()), "mvn_upsample_features")
    N.check(lib.mvn_upsample_features_backward(dctx_d.data_ptr(), T, mel_d.data_ptr(), F, w_d.data_ptr(), B, M, F, C, hop,
                                               T, dw.data_ptr(), db.data_ptr(), dmel.data_ptr(), F, scratch.data_ptr(), n,
                                               _stream()), "mvn_upsample_features_backward")
    guard.check("one tap")
    assert torch.equal(ctx[:, :, :T], old[:, :, :T])
    assert torch.equal(got["dw"][:, :, 0], dw) and torch.equal(got["dbias"], db) and torch.equal(got["dmel"], dmel)


class _LocalConvOnly(torch.nn.Module):
    """What ops.upsample_features reads of a model: local_channels, local_hop and local_conv."""

    def __init__(self, M, C, hop, k):
        super().__init__()
        self.local_channels, self.local_hop, self.local_window = M, hop, k
        self.local_conv = torch.nn.Conv1d(M, C, 2 * k + 1)


def test_python_entry_point_gives_the_bits_of_the_c_calls():
    from movenet_amd import ops
    B, M, F, C, hop, T, k = MULTI
    mel, w, bias, dctx = _case(MULTI)[:4]
    ctx0, dw0, db0, dmel0 = _contiguous(MULTI, zero_start=True)
    model = _LocalConvOnly(M, C, hop, k)
    with torch.no_grad():
        model.local_conv.weight.copy_(w)
        model.local_conv.bias.copy_(bias)
    model.to(DEV)
    feats = mel.to(DEV).requires_grad_(True)
    ctx = ops.upsample_features(model, feats, T)
    assert tuple(ctx.shape) == (B, C, T) and torch.equal(ctx.detach().cpu(), ctx0)
    ctx.backward(dctx.to(DEV))
    assert tuple(model.local_conv.weight.grad.shape) == (C, M, 2 * k + 1)
    assert torch.equal(model.local_conv.weight.grad.cpu(), dw0)
    assert torch.equal(model.local_conv.bias.grad.cpu(), db0)
    assert torch.equal(feats.grad.cpu(), dmel0)


def test_refusals_leave_the_outputs_untouched():
    B, M, F, C, hop, T, k = PLAIN
    mel, w, bias = _case(PLAIN)[:3]
    need = N.lib().mvn_upsample_features_scratch_floats(B, C, F)
    guard = _Guard()
    bad = [("even taps", dict(taps=2), "taps"), ("taps = 35", dict(taps=35), "taps"),
           ("a misaligned ctx_ld", dict(ctx_ld=T + 2), "multiple of 4"),
           ("too few frames", dict(frames=(T - 1) // hop), "too few frames"),
           ("a small scratch", dict(scratch_floats=need - 1), "scratch")]
    for name, over, word in bad:
        # (taps = 35 is refused before w is read: the (C, M, 3) weight stands in)
        rc, ctx, scratch = _run_forward(guard, mel, w, bias, hop, T, **over)
        assert rc == N.MVN_ERR_BAD_ARG, name
        assert "mvn_upsample_features_win" in N.last_error() and word in N.last_error(), (name, N.last_error())
        torch.cuda.synchronize()
        assert bool((ctx == SENTINEL).all()) and bool((scratch == SENTINEL).all()), name
    guard.check("refused mvn_upsample_features_win")
    # the backward refuses the same taps, with dw, dbias and dmel as they were
    lib = N.lib()
    dctx = _case(PLAIN)[3]
    bufs = dict(dw=guard.new((C, M, 2 * k + 1), SENTINEL, "dw"), dbias=guard.new((C,), SENTINEL, "dbias"),
                dmel=guard.new((B, M, F), SENTINEL, "dmel"))
    mel_d, w_d, dctx_d = guard.put(mel, "mel"), guard.put(w, "w"), guard.put(dctx, "dctx")
    scratch = guard.new((need,), SENTINEL, "scratch")
    for taps, frames, floats in ((2, F, need), (35, F, need), (3, (T - 1) // hop, need), (3, F, need - 1)):
        rc = lib.mvn_upsample_features_win_backward(dctx_d.data_ptr(), T, mel_d.data_ptr(), F, w_d.data_ptr(), B, M,
                                                    frames, C, taps, hop, T, bufs["dw"].data_ptr(),
                                                    bufs["dbias"].data_ptr(), bufs["dmel"].data_ptr(), F,
                                                    scratch.data_ptr(), floats, _stream())
        assert rc == N.MVN_ERR_BAD_ARG and "mvn_upsample_features_win_backward" in N.last_error(), (taps, frames, floats)
    torch.cuda.synchronize()
    assert all(bool((v == SENTINEL).all()) for v in bufs.values()) and bool((scratch == SENTINEL).all())
    guard.check("refused mvn_upsample_features_win_backward")
