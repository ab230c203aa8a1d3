"""GPU: mvn_upsample_features and its backward against float64 (tests/logmel_reference.upsample_features and torch
autograd of the same expression in float64).

Bounds: the ones tests/test_video_kernels_gpu.py uses for the video up-sampler -- forward max |err| / max |ref| below
1e-5 (its TOL_FWD), gradients below helpers.grad_bound of the deviation the same expression shows in fp32 on the CPU."""
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


def _forward(shape, guard, ctx_ld):
    lib = N.lib()
    B, M, F, C, hop, T = shape
    mel, w, bias = (guard.put(t, n) for t, n in zip(_case(shape)[:3], ("mel", "w", "bias")))
    ctx = guard.new((B, C, ctx_ld), SENTINEL, "ctx")
    n = lib.mvn_upsample_features_scratch_floats(B, C, F)
    scratch = guard.new((n,), float("nan"), "scratch")
    rc = lib.mvn_upsample_features(mel.data_ptr(), F, w.data_ptr(), bias.data_ptr(), B, M, F, C, hop, T, ctx.data_ptr(),
                                   ctx_ld, scratch.data_ptr(), n, _stream())
    return rc, mel, w, ctx


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


def _backward(shape, guard, want_dmel=True):
    lib = N.lib()
    B, M, F, C, hop, T = shape
    mel, w, _, dctx, g0, _, _ = _case(shape)
    mel_d, w_d, dctx_d = guard.put(mel, "mel"), guard.put(w, "w"), guard.put(dctx, "dctx")
    dw, db = guard.put(g0["dw"], "dw"), guard.put(g0["dbias"], "dbias")
    dmel = guard.new((B, M, F), float("nan"), "dmel") if want_dmel else None
    n = lib.mvn_upsample_features_scratch_floats(B, C, F)
    scratch = guard.new((n,), float("nan"), "scratch")
    N.check(lib.mvn_upsample_features_backward(dctx_d.data_ptr(), T, mel_d.data_ptr(), F, w_d.data_ptr(), B, M, F, C, hop,
                                               T, dw.data_ptr(), db.data_ptr(), dmel.data_ptr() if want_dmel else None,
                                               F, scratch.data_ptr(), n, _stream()), "mvn_upsample_features_backward")
    guard.check("mvn_upsample_features_backward")
    return dw, db, dmel


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
