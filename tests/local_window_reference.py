"""The windowed frame up-sampler (mvn_upsample_features_win) restated with torch's own operators, in
whatever precision its inputs come (the tests use float64, and float32 for the deviation ``helpers.grad_bound`` takes):

    proj = conv1d(pad(mel, (k, k), mode="replicate"), w) + bias          w (C, M, 2 k + 1), nn.Conv1d's layout
    ctx[b, c, t] = (1 - a) proj[b, c, j] + a proj[b, c, min(j + 1, F - 1)]     j = t // hop, a = (t % hop) / hop

-- the padding, not a clamped index, makes the window, and the interpolation is the expression of
``logmel_reference.upsample_features`` applied to the projected rows.  Gradients are torch autograd's."""
import torch
import torch.nn.functional as F


def project(mel, w, bias):
    """(B, M, F), (C, M, taps), (C) -> (B, C, F): the conv over the replicate-padded frames."""
    k = (w.shape[2] - 1) // 2
    padded = F.pad(mel, (k, k), mode="replicate") if k else mel
    return F.conv1d(padded, w, bias)


def upsample_features_win(mel, w, bias, hop, n_samples):
    mel, w, bias = (torch.as_tensor(v) for v in (mel, w, bias))
    assert w.dim() == 3 and w.shape[2] % 2 == 1
    proj = project(mel, w, bias)
    frames = proj.shape[2]
    t = torch.arange(n_samples)
    j = t // hop
    j1 = torch.clamp(j + 1, max=frames - 1)
    a = ((t % hop).to(proj.dtype) / hop)[None, None, :]
    return (1.0 - a) * proj[:, :, j] + a * proj[:, :, j1]


def reference(mel, w, bias, dctx, hop, n_samples, dtype=torch.float64):
    """ctx and the gradients of <ctx, dctx> in ``dtype``: dict(ctx, dmel, dw, dbias)."""
    q = [v.detach().to(dtype).clone().requires_grad_(True) for v in (mel, w, bias)]
    ctx = upsample_features_win(*q, hop, n_samples)
    ctx.backward(dctx.to(dtype))
    return dict(ctx=ctx.detach(), dmel=q[0].grad, dw=q[1].grad, dbias=q[2].grad)


def frame_gradient(dctx, frames, hop):
    """dP (B, C, F) of a dctx (B, C, T): what the interpolation hands back to the projected rows."""
    proj = torch.zeros(dctx.shape[0], dctx.shape[1], frames, dtype=dctx.dtype, requires_grad=True)
    t = torch.arange(dctx.shape[2])
    j = t // hop
    j1 = torch.clamp(j + 1, max=frames - 1)
    a = ((t % hop).to(dctx.dtype) / hop)[None, None, :]
    ((1.0 - a) * proj[:, :, j] + a * proj[:, :, j1]).backward(dctx)
    return proj.grad
