"""GPU: mvn_upsample_features and its backward against float64 (tests/logmel_reference.upsample_features and torch
autograd of the same expression in float64).

Bounds: the ones tests/test_video_kernels_gpu.py uses for the video up-sampler -- forward max |err| / max |ref| below
1e-5 (its TOL_FWD), gradients below helpers.grad_bound of the deviation the same expression shows in fp32 on the CPU.
Everything else here is bit equality: two runs, row strides above the row lengths against the contiguous call, a
translation by one workgroup, the Python entry point against the C calls.  Measured: DESIGN 4.5d."""
import functools

import pytest
import torch

import logmel_reference as R
from helpers import DEV, SENTINEL, _Guard, grad_bound
from movenet_amd import _native as N

pytestmark = pytest.mark.gpu
TOL_FWD = 1e-5
# (B, M, F, C, hop, T): T - 1 a multiple of hop (9 - 1 at hop 1, 1000 - 1 is not at 256, 100 - 1 is not at 16) ...
SHAPES = [(2, 5, 7, 16, 16, 100), (1, 80, 5, 64, 256, 1000), (3, 8, 9, 32, 1, 9), (2, 8, 12, 128, 16, 100),
          (2, 5, 7, 16, 16, 97)]   # ... and 97 - 1 = 6 x 16 is
# Past the first workgroup of every kernel (64 frames per uf_project / uf_dmel workgroup and per pass of the uf_dw loop,
# 16 per uf_dp segment, 1024 columns per uf_interp workgroup):
MULTI = (2, 5, 71, 16, 16, 1101)   # 69 frames needed of 71: a surplus frame; 5 uf_dp segments, the last of 7 frames; a
#                                    second pass of the uf_dw loop; two interpolation workgroups, a one-column tail
SHAPES += [
    MULTI,
    (1, 4, 65, 4, 16, 1024),    # T exactly one interpolation workgroup, one frame past a project workgroup
    (1, 4, 66, 4, 16, 1025),    # one column in a second interpolation workgroup
    (2, 6, 21, 8, 101, 2050),   # hop % 4 != 0: float4 groups straddle frames with a != 0; four passes of the uf_dp lane
                                # loop; F = the 21 frames needed (the last frame's (1 - a) + a); the tail in workgroup 1
    (1, 3, 33, 2, 7, 225),      # hop 7: groups straddle on almost every frame; the third uf_dp segment holds one frame
]


def _err(got, want):
    return ((got.double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-30)).item()


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _reference(mel, w, bias, dctx, hop, T, dtype):
    q = [v.detach().to(dtype).clone().requires_grad_(True) for v in (mel, w, bias)]
    ctx = R.upsample_features(*q, hop, T)
    ctx.backward(dctx.to(dtype))
    return dict(ctx=ctx.detach(), dmel=q[0].grad, dw=q[1].grad, dbias=q[2].grad)


@functools.lru_cache(maxsize=None)
def _case(shape):
    B, M, F, C, hop, T = shape
    g = torch.Generator().manual_seed(sum(p * v for p, v in zip((7, 11, 13, 17, 19, 23), shape)))
    mel, w, bias = torch.randn(B, M, F, generator=g), torch.randn(C, M, generator=g) / M ** 0.5, torch.randn(C, generator=g)
    dctx = torch.randn(B, C, T, generator=g)
    g0 = dict(dw=torch.randn(C, M, generator=g), dbias=torch.randn(C, generator=g))   # what the buffers hold before
    ref = _reference(mel, w, bias, dctx, hop, T, torch.float64)
    ref32 = _reference(mel, w, bias, dctx, hop, T, torch.float32)
    return mel, w, bias, dctx, g0, ref, {k: _err(ref32[k], ref[k]) for k in ref}


def _padded(guard, t, pad, name):
    """``t`` (B, R, L) as the first L columns of the rows of a (B, R, L + pad) buffer whose other columns hold NaN."""
    if pad == 0:
        return guard.put(t, name)
    buf = guard.new((t.shape[0], t.shape[1], t.shape[2] + pad), float("nan"), name)
    buf[:, :, :t.shape[2]].copy_(t)
    return buf


def _run_forward(guard, mel, w, bias, hop, T, ctx_ld, mel_pad=0):
    lib = N.lib()
    (B, M, F), C = mel.shape, w.shape[0]
    mel, w, bias = _padded(guard, mel, mel_pad, "mel"), guard.put(w, "w"), guard.put(bias, "bias")
    ctx = guard.new((B, C, ctx_ld), SENTINEL, "ctx")
    n = lib.mvn_upsample_features_scratch_floats(B, C, F)
    scratch = guard.new((n,), float("nan"), "scratch")
    rc = lib.mvn_upsample_features(mel.data_ptr(), F + mel_pad, w.data_ptr(), bias.data_ptr(), B, M, F, C, hop, T,
                                   ctx.data_ptr(), ctx_ld, scratch.data_ptr(), n, _stream())
    return rc, mel, w, ctx


def _forward(shape, guard, ctx_ld, mel_pad=0):
    mel, w, bias = _case(shape)[:3]
    return _run_forward(guard, mel, w, bias, shape[4], shape[5], ctx_ld, mel_pad)


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_against_float64(shape):
    B, M, F, C, hop, T = shape
    ref = _case(shape)[5]
    guard = _Guard()
    ld = (T + 3) // 4 * 4 + 8
    rc, _, _, ctx = _forward(shape, guard, ld)
    N.check(rc, "mvn_upsample_features")
    guard.check("mvn_upsample_features")
    assert bool((ctx[:, :, T:] == SENTINEL).all()), "columns past T were written"
    e = _err(ctx[:, :, :T], ref["ctx"])
    print(f"upsample_features forward {shape}: {e:.2e}")
    assert e < TOL_FWD, (shape, e)
    if hop == 1:   # the interpolation is the identity: the frame-rate product itself
        mel, w, bias = _case(shape)[:3]
        want = torch.einsum("cm,bmf->bcf", w.double(), mel.double()) + bias.double()[None, :, None]
        assert _err(ctx[:, :, :T], want[:, :, :T]) < TOL_FWD


def test_misaligned_ctx_ld_is_refused_with_the_output_untouched():
    shape = SHAPES[0]
    guard = _Guard()
    for ld in (101, 102, 103):
        rc, _, _, ctx = _forward(shape, guard, ld)
        assert rc == N.MVN_ERR_BAD_ARG and "multiple of 4" in N.last_error()
        torch.cuda.synchronize()
        assert bool((ctx == SENTINEL).all())
    guard.check("refused mvn_upsample_features")


def _run_backward(guard, mel, w, dctx, dw0, db0, hop, T, want_dmel=True, pads=(0, 0, 0), dmel_fill=float("nan")):
    """``pads``: what dctx_ld, mel_ld and dmel_ld exceed T, F and F by."""
    lib = N.lib()
    (B, M, F), C = mel.shape, w.shape[0]
    mel_d, w_d, dctx_d = _padded(guard, mel, pads[1], "mel"), guard.put(w, "w"), _padded(guard, dctx, pads[0], "dctx")
    dw, db = guard.put(dw0, "dw"), guard.put(db0, "dbias")
    dmel = guard.new((B, M, F + pads[2]), dmel_fill, "dmel") if want_dmel else None
    n = lib.mvn_upsample_features_scratch_floats(B, C, F)
    scratch = guard.new((n,), float("nan"), "scratch")
    N.check(lib.mvn_upsample_features_backward(dctx_d.data_ptr(), T + pads[0], mel_d.data_ptr(), F + pads[1],
                                               w_d.data_ptr(), B, M, F, C, hop, T, dw.data_ptr(), db.data_ptr(),
                                               dmel.data_ptr() if want_dmel else None, F + pads[2], scratch.data_ptr(),
                                               n, _stream()), "mvn_upsample_features_backward")
    guard.check("mvn_upsample_features_backward")
    return dw, db, dmel


def _backward(shape, guard, want_dmel=True, **kw):
    mel, w, _, dctx, g0, _, _ = _case(shape)
    return _run_backward(guard, mel, w, dctx, g0["dw"], g0["dbias"], shape[4], shape[5], want_dmel, **kw)


@pytest.mark.parametrize("shape", SHAPES)
def test_backward_against_float64_autograd(shape):
    B, M, F, C, hop, T = shape
    _, _, _, _, g0, ref, dev = _case(shape)
    dw, db, dmel = _backward(shape, _Guard())
    # dW and dbias were accumulated INTO what the buffers held
    got = dict(dw=dw.cpu() - g0["dw"], dbias=db.cpu() - g0["dbias"], dmel=dmel.cpu())
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    worst = {k: _err(got[k], ref[k]) for k in got}
    print(f"upsample_features backward {shape}: " + " ".join(f"{k} {v:.2e}/{grad_bound(dev[k]):.1e}" for k, v in worst.items()))
    for k, e in worst.items():
        assert e < grad_bound(dev[k]), (shape, k, e, dev[k])
    need = (T - 1) // hop + 1
    if F > need + 1:   # frames no column touches: exactly 0 (frame `need` still gets the a-weights of frame need - 1)
        assert bool((ref["dmel"][:, :, need + 1:] == 0).all())
        assert bool((dmel[:, :, need + 1:] == 0).all()), "surplus frames received a gradient"
    # two runs: the same bits; and without dmel the other two are the same bits again
    dw2, db2, dmel2 = _backward(shape, _Guard())
    assert torch.equal(dw, dw2) and torch.equal(db, db2) and torch.equal(dmel, dmel2)
    dw3, db3, _ = _backward(shape, _Guard(), want_dmel=False)
    assert torch.equal(dw, dw3) and torch.equal(db, db3)


def test_surplus_frames_leave_dw_unaffected():
    """(2, 8, 12, 128, 16, 100) against the same data cut to the 8 frames its columns reach (7 needed + the one the last
    hop leans on): the surplus frames' dP is 0, so dW and dbias are the same bits."""
    shape = SHAPES[3]
    B, M, F, C, hop, T = shape
    mel, w, _, dctx, g0, _, _ = _case(shape)
    lib = N.lib()

    def run(frames):
        mel_d, w_d, dctx_d = mel[:, :, :frames].contiguous().to(DEV), w.to(DEV), dctx.to(DEV)
        dw, db = g0["dw"].to(DEV), g0["dbias"].to(DEV)
        n = lib.mvn_upsample_features_scratch_floats(B, C, frames)
        scratch = torch.empty(n, device=DEV)
        N.check(lib.mvn_upsample_features_backward(dctx_d.data_ptr(), T, mel_d.data_ptr(), frames, w_d.data_ptr(), B, M,
                                                   frames, C, hop, T, dw.data_ptr(), db.data_ptr(), None, frames,
                                                   scratch.data_ptr(), n, _stream()), "backward")
        torch.cuda.synchronize()
        return dw.cpu(), db.cpu()
    full, cut = run(F), run(8)
    assert torch.equal(full[0], cut[0]) and torch.equal(full[1], cut[1])


@functools.lru_cache(maxsize=None)
def _contiguous(shape, zero_start=False):
    """The contiguous C calls on ``shape``: (ctx[:, :, :T], dW, dbias, dmel) on the CPU; ``zero_start``: dW and dbias
    accumulated into zeros, as ops.upsample_features does."""
    T = shape[5]
    mel, w, bias, dctx, g0 = _case(shape)[:5]
    guard = _Guard()
    rc, _, _, ctx = _run_forward(guard, mel, w, bias, shape[4], T, (T + 3) // 4 * 4)
    N.check(rc, "mvn_upsample_features")
    guard.check("mvn_upsample_features")
    dw0, db0 = (torch.zeros_like(g0[k]) if zero_start else g0[k] for k in ("dw", "dbias"))
    dw, db, dmel = _run_backward(guard, mel, w, dctx, dw0, db0, shape[4], T)
    return ctx[:, :, :T].cpu(), dw.cpu(), db.cpu(), dmel.cpu()


def test_row_strides_that_differ_from_the_row_lengths():
    """mel_ld = F + 5, dctx_ld = T + 7, dmel_ld = F + 3 on the multi-workgroup shape, NaN in the padding columns of the
    inputs: the same bits as the contiguous calls, the padding columns of dmel untouched."""
    B, M, F, C, hop, T = MULTI
    ctx0, dw0, db0, dmel0 = _contiguous(MULTI)
    guard = _Guard()
    rc, mel, _, ctx = _forward(MULTI, guard, (T + 3) // 4 * 4, mel_pad=5)
    N.check(rc, "mvn_upsample_features")
    guard.check("mvn_upsample_features (mel_ld = F + 5)")
    assert tuple(mel.shape) == (B, M, F + 5) and bool(torch.isnan(mel[:, :, F:]).all())
    assert bool(torch.isfinite(ctx[:, :, :T]).all()) and torch.equal(ctx[:, :, :T].cpu(), ctx0)
    assert bool((ctx[:, :, T:] == SENTINEL).all())
    dw, db, dmel = _backward(MULTI, guard, pads=(7, 5, 3), dmel_fill=SENTINEL)   # (checks the guards itself)
    assert tuple(dmel.shape) == (B, M, F + 3)
    assert all(bool(torch.isfinite(v).all()) for v in (dw, db, dmel))
    assert torch.equal(dw.cpu(), dw0) and torch.equal(db.cpu(), db0) and torch.equal(dmel[:, :, :F].cpu(), dmel0)
    assert bool((dmel[:, :, F:] == SENTINEL).all()), "padding columns of dmel were written"


def test_a_translation_by_one_workgroup_gives_the_same_bits():
    """hop 16, T = 2048, F = 129: frames and columns moved by 64 frames = 1024 columns = one uf_interp workgroup, one
    uf_project / uf_dmel workgroup, four uf_dp segments.  Nothing in a column's or a frame's arithmetic depends on
    where it sits, so the moved results are the same bits -- no tolerance."""
    B, M, F, C, hop, T = 1, 4, 129, 4, 16, 2048
    shift_f, shift_t = 64, 1024
    g = torch.Generator().manual_seed(20480129)
    mel_a, w = torch.randn(B, M, F, generator=g), torch.randn(C, M, generator=g) / M ** 0.5
    bias = torch.randn(C, generator=g)
    mel_b = torch.randn(B, M, F, generator=g)
    mel_b[:, :, shift_f:] = mel_a[:, :, :F - shift_f]
    guard = _Guard()
    ctx = []
    for mel in (mel_a, mel_b):
        rc, _, _, out = _run_forward(guard, mel, w, bias, hop, T, T)
        N.check(rc, "mvn_upsample_features")
        ctx.append(out)
    guard.check("mvn_upsample_features")
    # column t < 1024 reads frames t // 16 and t // 16 + 1 <= 64 of a: frames <= 128 of b, in the next workgroups
    assert bool(torch.isfinite(ctx[0]).all()) and float(ctx[0][:, :, :shift_t].abs().max()) > 0
    assert torch.equal(ctx[1][:, :, shift_t:], ctx[0][:, :, :shift_t])
    assert not torch.equal(ctx[1][:, :, :shift_t], ctx[0][:, :, :shift_t])   # (the other frames of b are other values)
    # backward: dctx lives on [0, 1024) in a, the same values on [1024, 2048) in b
    dctx_a = torch.zeros(B, C, T)
    dctx_a[:, :, :shift_t] = torch.randn(B, C, shift_t, generator=g)
    dctx_b = torch.roll(dctx_a, shift_t, dims=2)
    assert bool((dctx_b[:, :, :shift_t] == 0).all()) and torch.equal(dctx_b[:, :, shift_t:], dctx_a[:, :, :shift_t])
    zw, zb = torch.zeros(C, M), torch.zeros(C)
    dmel_a = _run_backward(guard, mel_a, w, dctx_a, zw, zb, hop, T)[2]
    dmel_b = _run_backward(guard, mel_a, w, dctx_b, zw, zb, hop, T)[2]
    # frames 1 .. 63 of a: both column ranges [(j - 1) hop, (j + 1) hop) inside the window, as those of j + 64 are in b
    lo, hi = 1, shift_f - 1
    assert float(dmel_a[:, :, lo:hi + 1].abs().min()) > 0
    assert torch.equal(dmel_b[:, :, lo + shift_f:hi + shift_f + 1], dmel_a[:, :, lo:hi + 1])
    # frames no non-zero column touches: a's columns end at 1023 = frame 64's a-weights; b's begin at 1024 = frame 64
    assert bool((dmel_a[:, :, shift_f + 1:] == 0).all()) and bool((dmel_b[:, :, :shift_f] == 0).all())
    assert float(dmel_a[:, :, shift_f].abs().max()) > 0 and float(dmel_b[:, :, shift_f].abs().max()) > 0


class _LocalConvOnly(torch.nn.Module):
    """What ops.upsample_features reads of a model: local_channels, local_hop and the 1 x 1 local_conv."""

    def __init__(self, M, C, hop):
        super().__init__()
        self.local_channels, self.local_hop = M, hop
        self.local_conv = torch.nn.Conv1d(M, C, 1)


def test_python_entry_point_gives_the_bits_of_the_c_calls():
    from movenet_amd import ops
    B, M, F, C, hop, T = MULTI
    mel, w, bias, dctx = _case(MULTI)[:4]
    ctx0, dw0, db0, dmel0 = _contiguous(MULTI, zero_start=True)
    model = _LocalConvOnly(M, C, hop)
    with torch.no_grad():
        model.local_conv.weight.copy_(w[:, :, None])
        model.local_conv.bias.copy_(bias)
    model.to(DEV)
    feats = mel.to(DEV).requires_grad_(True)
    ctx = ops.upsample_features(model, feats, T)
    assert tuple(ctx.shape) == (B, C, T) and torch.equal(ctx.detach().cpu(), ctx0)
    ctx.backward(dctx.to(DEV))
    assert torch.equal(model.local_conv.weight.grad[:, :, 0].cpu(), dw0)
    assert torch.equal(model.local_conv.bias.grad.cpu(), db0)
    assert torch.equal(feats.grad.cpu(), dmel0)
