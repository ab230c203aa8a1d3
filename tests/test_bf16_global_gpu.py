"""GPU: labelled training in bf16 -- ``global_path = "bias"`` under ``forward_precision = "bf16"`` (DESIGN 4.3d, 7.3;
mvn_forward_bf16_global / mvn_backward_bf16_global, backward form MVN_BWD_FORM_BF16_GLOBAL).

The layers' products are those of the audio-only bf16 mode; the label's term gb[l][b] = [Wcf_l e_b + bcf_l | Wcg_l e_b +
bcg_l] is fp32, starts the f | g accumulators, and its gradients are the fp32 row sums of df | dg formed inside the layer
kernel.  Yardsticks: the fp32 oracle fed ``context = e[:, :, None]`` (test_global_conditioning_gpu.py's) and
tests/bf16_global_emulation.py, the same rounding points on the oracle's arithmetic.  The criteria are those of
test_bf16_train_gpu.py, restated here and applied to EVERY parameter, the four context tensors of every layer and
``global_embedding.weight`` included:
  logits      rel_err(got, oracle) <= 2 x rel_err(emulation, oracle)
  gradients   cosine with the oracle's >= min(0.99, the emulation's worst - 0.005);
              norm within max(3 %, 1.5 x the emulation's worst norm deviation) of the oracle's

Shapes (layers, stacks, Q, B, T):
  a  2 x 2, 64, 2, 300      one tile per chunk, several chunks per sequence, T no multiple of 64
  b  2 x 2, 64, 16, 1100    two tiles per chunk at 256 CUs (fb_chunks): the per-thread row sums carry across tiles
  c  10 x 1, 64, 2, 1025    the last layer's dilation (512) exceeds its valid span (2 columns)
  d  10 x 3, 256, 2, 3073   one output column; the slabs take the caller's scratch (da1 is far too small)
"""
import functools
import os
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bf16_global_emulation as EG
from helpers import _Guard, one_hot, rel_err, synthetic_indices
from movenet_amd import _native as N
from movenet_amd import ops
from movenet_amd.utils.weights import make_state_dict
from oracle import wavenet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = 4
CLASSES = [2, 2, 0, 1, 3, 0, 2, 1, 1, 3, 0, 0, 2, 3, 1, 2]  # (the first two repeat: every batch has a repeated class)
SHAPES = {"a": (2, 2, 64, 2, 300), "b": (2, 2, 64, 16, 1100), "c": (10, 1, 64, 2, 1025), "d": (10, 3, 256, 2, 3073)}
# test 1 compares with the AUDIO-ONLY bf16 model, bit for bit, every tensor.  A layer's weight and bias gradients are
# sums over its workgroups' partials in chunk order; mvn_backward_bf16_global never places more workgroups than
# mvn_backward_bf16 would at the same shape (sequence.hip), so wherever the audio-only pass runs both cut a sequence
# into the same chunks.  (b) runs as the issue states it.  At (a) the audio-only pass does not run: its slabs live in
# the (B, Q, Sp) da1 tensor or the forward's z scratch, 40960 floats each at Q = 64 against two workgroups' 49408, and
# it refuses, as it always has.  The layer kernels never see Q, so (a) is compared at Q = 256, where da1
# holds three chunks per sequence: same layers, batch and length, T no multiple of 64.
SHAPES_VS_AUDIO_ONLY = {"a_q256": (2, 2, 256, 2, 300), "b": SHAPES["b"]}
NAN = float("nan")


def _cfg(layer_size, stack_size, Q, C=64):
    return dict(layer_size=layer_size, stack_size=stack_size, input_channels=Q, residual_channels=C, skip_channels=C)


def _embedding(C=64, seed=99):
    return torch.randn(G, C, generator=torch.Generator().manual_seed(seed))


def _model(cfg, full, E=None, precision="bf16", path="bias", **kw):
    from movenet_amd.wavenet import WaveNet
    m = WaveNet(**cfg, global_classes=0 if E is None else E.shape[0], **kw)
    m.load_state_dict(dict(full) if E is None else {**full, "global_embedding.weight": E}, strict=True)
    m.forward_precision = precision
    if E is not None:
        m.global_path = path
    return m.to(DEV)


@functools.lru_cache(maxsize=None)
def _case(name, seed=7):
    ls, ss, Q, B, T = SHAPES_VS_AUDIO_ONLY[name] if name in SHAPES_VS_AUDIO_ONLY else SHAPES[name]
    cfg = _cfg(ls, ss, Q)
    full = make_state_dict(**cfg, seed=seed)
    sd = {k: v for k, v in full.items() if not k.startswith("video_")}
    dims = O.Dims(**cfg)
    assert T >= dims.receptive_fields + 1
    x = one_hot(synthetic_indices(B, T, Q, seed + 1), Q)
    up = torch.randn(B, Q, T - dims.receptive_fields, generator=torch.Generator().manual_seed(11))
    return cfg, dims, full, sd, x, torch.tensor(CLASSES[:B]), up


def _cos(a, b) -> float:
    a, b = a.double().flatten(), b.double().flatten()
    return (a @ b / (a.norm() * b.norm()).clamp_min(1e-300)).item()


def _norm_dev(a, ref) -> float:
    return abs(a.double().norm().item() - ref.double().norm().item()) / ref.double().norm().item()


def _check_grads(got, oracle, emu, what):
    """test_bf16_train_gpu.py's rule: every oracle gradient's cosine >= min(0.99, emulation's worst - 0.005); its norm
    within 3 % of the oracle's, or within 1.5 x the emulation's worst norm deviation where that is larger."""
    assert sorted(got) == sorted(oracle), (what, sorted(set(got) ^ set(oracle)))
    emu_min = min(_cos(emu[k], oracle[k]) for k in oracle)
    floor = min(0.99, emu_min - 0.005)
    worst = min((_cos(got[k].cpu(), oracle[k]), k) for k in oracle)
    tol = max(0.03, 1.5 * max(_norm_dev(emu[k], oracle[k]) for k in oracle))
    devs = {k: _norm_dev(got[k].cpu(), oracle[k]) for k in oracle}
    k_dev = max(devs, key=devs.get)
    print(f"{what}: worst cosine {worst[0]:.5f} ({worst[1]}; emulation {emu_min:.5f}, floor {floor:.5f}); worst norm "
          f"deviation {devs[k_dev]:.4f} ({k_dev}; bound {tol:.4f})")
    assert worst[0] >= floor, (what, worst, emu_min)
    for k in oracle:
        assert devs[k] <= tol, (what, k, devs[k], tol)
    return worst[0], emu_min


def _reference(sd, dims, E, x, e_of, kind, up, logits_fn):
    """(value, {name: gradient}, de) of ``logits_fn(params, e)`` under the trainer's loss or the upstream gradient ``up``;
    ``e_of(E)`` -> the (B, C) global vectors.  The gradient of E is filed under the model's parameter name."""
    params = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    Ep = E.clone().requires_grad_(True)
    e = e_of(Ep)
    e.retain_grad()
    lg = logits_fn(params, e)[:, :, :-1]
    if kind == "loss":
        target = x[:, :, dims.receptive_fields:].argmax(1)
        F.cross_entropy(F.softmax(lg, dim=1), target).backward()
    else:
        (lg * up).sum().backward()
    grads = {k: p.grad for k, p in params.items() if p.grad is not None}
    grads["global_embedding.weight"] = Ep.grad
    return lg.detach(), grads, e.grad


def _oracle_and_emulation(sd, dims, E, x, e_of, kind, up):
    T = x.shape[2]
    ref = _reference(sd, dims, E, x, e_of, kind, up,
                     lambda p, e: O.logits_full(p, dims, x, context=e[:, :, None].expand(-1, -1, T)))
    emu = _reference(sd, dims, E, x, e_of, kind, up, lambda p, e: EG.logits(p, dims, x, e))
    return ref, emu


@functools.lru_cache(maxsize=None)
def _refs(name, kind):
    cfg, dims, full, sd, x, feats, up = _case(name)
    return _oracle_and_emulation(sd, dims, _embedding(), x, lambda Ep: Ep[feats], kind, up)


def _device_step(m, x, feats, kind, up):
    m.zero_grad(set_to_none=True)
    if kind == "loss":
        loss, _acc, _probs = m(x.to(DEV), None, feats.to(DEV), return_loss=True)
        loss.backward()
        out = None
    else:
        out = m(x.to(DEV), None, feats.to(DEV), output_unnormalized=False)
        (out * up.to(DEV)).sum().backward()
        out = out.detach().cpu()
    form = N.lib().mvn_last_backward_form()
    return out, {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}, form


# ---- 1. a zero label term is the audio-only model, to the bit --------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SHAPES_VS_AUDIO_ONLY))
def test_zero_label_term_equals_audio_only_to_the_bit(name):
    """Zero context-conv weights and biases, any labels: gb = 0, so the GLOBAL kernels must give the audio-only
    kernels' bits in the logits and in every non-context gradient (torch.equal: -0 counts as 0) -- everything in them
    but the bias start and the row sums.  The context-conv gradients, sum_b r (x) e_b and sum_b r, are non-zero."""
    cfg, dims, full, sd, x, feats, up = _case(name)
    zeroed = {k: (torch.zeros_like(v) if "context_conv" in k else v) for k, v in full.items()}
    E = _embedding()
    labelled, plain = _model(cfg, zeroed, E).train(), _model(cfg, zeroed).train()
    for kind in ("loss", "logits"):
        out_l, g_l, form_l = _device_step(labelled, x, feats, kind, up)
        assert form_l == N.BWD_FORM_BF16_GLOBAL
        plain.zero_grad(set_to_none=True)
        if kind == "loss":
            loss, _, _ = plain(x.to(DEV), return_loss=True)
            loss.backward()
        else:
            out_p = plain(x.to(DEV), output_unnormalized=False)
            (out_p * up.to(DEV)).sum().backward()
            assert torch.equal(out_l, out_p.detach().cpu())
        assert N.lib().mvn_last_backward_form() == N.BWD_FORM_BF16
        g_p = {k: p.grad for k, p in plain.named_parameters() if p.grad is not None}
        assert g_p and not any("context_conv" in k for k in g_p)
        for k, g in g_p.items():
            assert torch.equal(g_l[k], g), (kind, k)
        ctx = [k for k in g_l if "context_conv" in k]
        assert len(ctx) == 4 * dims.n_layers
        for k in ctx:
            assert bool(torch.isfinite(g_l[k]).all()) and float(g_l[k].abs().max()) > 0.0, (kind, k)
        # de = sum_l Wc^T r is zero with zero weights, and so is dE
        assert float(g_l["global_embedding.weight"].abs().max()) == 0.0


# ---- 2. against the oracle and the emulation --------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["loss", "logits"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_against_oracle_and_emulation(monkeypatch, name, kind):
    """Measured on an MI355X ("bf16"): the worst cosine and the logits error of each shape equal the
    emulation's to three digits or better; printed here with pytest -s."""
    monkeypatch.setenv("MOVENET_DEBUG_GUARD", "1")  # guard bands behind every scratch tensor of both passes
    cfg, dims, full, sd, x, feats, up = _case(name)
    (lg_ref, g_ref, _), (lg_emu, g_emu, _) = _refs(name, kind)
    m = _model(cfg, full, _embedding()).train()
    out, got, form = _device_step(m, x, feats, kind, up)
    assert form == N.BWD_FORM_BF16_GLOBAL, form
    if out is not None:
        e_got, e_emu = rel_err(out, lg_ref), rel_err(lg_emu, lg_ref)
        print(f"{name}/{kind}: logits rel. err bf16 HIP {e_got:.2e}, emulation {e_emu:.2e}")
        assert e_got <= 2 * e_emu, (e_got, e_emu)
    _check_grads(got, g_ref, g_emu, f"{name}/{kind}")
    absent = [c for c in range(G) if c not in feats.tolist()]
    dE = got["global_embedding.weight"]
    assert torch.equal(dE[absent], torch.zeros_like(dE[absent]))


# ---- 3. label dropout and mixed rows ------------------------------------------------------------------------------
def test_dropped_row_and_soft_rows():
    """B = 3 soft rows, the middle one dropped (its e is zero, as a ``global_dropout_mask`` row makes it): the criteria
    of test 2 through the module, and -- with e itself as the differentiated argument -- the dropped row's de, which is
    still sum_l Wc^T r of ITS row sums."""
    cfg = _cfg(2, 2, 64)
    full = make_state_dict(**cfg, seed=13)
    sd = {k: v for k, v in full.items() if not k.startswith("video_")}
    dims, E, B, T = O.Dims(**cfg), _embedding(), 3, 300
    rows = torch.softmax(torch.randn(B, G, generator=torch.Generator().manual_seed(3)), dim=1)
    keep = torch.tensor([1.0, 0.0, 1.0])
    x = one_hot(synthetic_indices(B, T, 64, 14), 64)
    up = torch.randn(B, 64, T - dims.receptive_fields, generator=torch.Generator().manual_seed(11))
    (lg_ref, g_ref, de_ref), (lg_emu, g_emu, de_emu) = _oracle_and_emulation(
        sd, dims, E, x, lambda Ep: (rows @ Ep) * keep[:, None], "logits", up)
    m = _model(cfg, full, E).train()
    m.global_dropout_mask = lambda batch: keep  # (what the module draws when global_dropout > 0)
    out, got, form = _device_step(m, x, rows, "logits", up)
    assert form == N.BWD_FORM_BF16_GLOBAL
    assert rel_err(out, lg_ref) <= 2 * rel_err(lg_emu, lg_ref)
    _check_grads(got, g_ref, g_emu, "dropped + soft rows")
    # e as a leaf: its gradient row by row
    e = ((rows @ E) * keep[:, None]).to(DEV).requires_grad_(True)
    m.zero_grad(set_to_none=True)
    res = ops.wavenet_forward(m, x.to(DEV), output_unnormalized=False, gvec=e)
    (res * up.to(DEV)).sum().backward()
    assert float(e.detach()[1].abs().max()) == 0.0 and float(e.grad[1].abs().max()) > 0.0
    _check_grads({f"de[{b}]": e.grad[b] for b in range(B)}, {f"de[{b}]": de_ref[b] for b in range(B)},
                 {f"de[{b}]": de_emu[b] for b in range(B)}, "de rows")


# ---- 4. determinism and form -----------------------------------------------------------------------------------
def test_determinism_and_forms():
    cfg, dims, full, sd, x, feats, up = _case("b")
    m = _model(cfg, full, _embedding()).train()
    out1, g1, form1 = _device_step(m, x, feats, "logits", up)
    out2, g2, form2 = _device_step(m, x, feats, "logits", up)
    assert form1 == form2 == N.BWD_FORM_BF16_GLOBAL
    assert torch.equal(out1, out2) and sorted(g1) == sorted(g2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    # fp32: "bias" is the fast path "auto" prefers, required instead of preferred
    m32 = _model(cfg, full, _embedding(), precision="fp32").train()
    out_b, g_b, form_b = _device_step(m32, x, feats, "logits", up)
    m32.global_path = "auto"
    out_a, g_a, form_a = _device_step(m32, x, feats, "logits", up)
    assert form_b == form_a == N.BWD_FORM_ONE_GLOBAL
    assert torch.equal(out_b, out_a) and sorted(g_b) == sorted(g_a)
    for k in g_b:
        assert torch.equal(g_b[k], g_a[k]), k
    assert not torch.equal(out_b, out1)  # (the bf16 kernels ran above)


# ---- 5. the C ABI on poisoned buffers -------------------------------------------------------------------------------
def _bits(t):
    return t.detach().reshape(-1).view(torch.int32).clone()


def test_c_abi_on_poisoned_buffers():
    """mvn_forward_bf16_global / mvn_backward_bf16_global through ctypes at shape (a), every buffer NaN-filled with a
    sentinel band in front of it and behind it (helpers._Guard, as test_decoder_abi_gpu.py does).  A refused call
    returns the documented code and leaves every buffer's bits alone; an accepted one writes rowsum in full and
    nothing outside the documented outputs, and its gradients -- into zero-filled tensors, with the scratch size ops.py
    passes -- are those of the module's step, to the bit."""
    lib = N.lib()
    cfg, dims_o, full, sd, x, feats, up = _case("a")
    ls, ss, Q, B, T = SHAPES["a"]
    C = K = 64
    L, S = dims_o.n_layers, T - dims_o.receptive_fields + 1
    E = _embedding()
    m = _model(cfg, full, E).train()
    _, want, form = _device_step(m, x, feats, "logits", up)
    assert form == N.BWD_FORM_BF16_GLOBAL
    stream = torch.cuda.current_stream(DEV).cuda_stream

    g = _Guard(front=True)
    dims = N.make_dims(ls, ss, Q, C, K)
    Tp, Sp = lib.mvn_padded_len(T), lib.mvn_padded_len(S + 31)
    pd = {k: g.put(v.to(DEV), k) for k, v in sd.items()}
    params, _keep = ops.pack_params(dims, pd, L)
    index = g.put(x.argmax(1).to(DEV, torch.int32), "index")
    e = g.put(E[feats].to(DEV), "e")
    gbias = g.new((L, B, 128), NAN, "gbias")
    fwd = dict(acts=g.new((L + 1, B, C, Tp), NAN, "acts"), th=g.new((L, B, C, Tp), NAN, "th"),
               sg=g.new((L, B, C, Tp), NAN, "sg"), z=g.new((B, C, Tp), NAN, "z"), skip=g.new((B, K, Sp), NAN, "skip"),
               a1=g.new((B, Q, Sp), NAN, "a1"))
    out = g.new((B, Q, S - 1), NAN, "out")
    ctx = g.new((B, C, Tp), NAN, "ctx")

    def fwd_struct(with_ctx=False):
        return N.FwdBuffers(fwd["acts"].data_ptr(), fwd["th"].data_ptr(), fwd["sg"].data_ptr(), fwd["z"].data_ptr(),
                            fwd["skip"].data_ptr(), fwd["a1"].data_ptr(), ctx.data_ptr() if with_ctx else None,
                            Tp if with_ctx else 0, None, 0)

    def forward(d=dims, with_ctx=False, gb=gbias):
        return lib.mvn_forward_bf16_global(d, params, index.data_ptr(), index.stride(0), B, T, fwd_struct(with_ctx),
                                           out.data_ptr(), 0, 1, 1, None if gb is None else gb.data_ptr(), stream)

    def snapshot(tensors):
        torch.cuda.synchronize()
        return {k: _bits(v) for k, v in tensors.items()}

    def unchanged(before, tensors, what):
        g.check(what)
        for k, v in tensors.items():
            assert torch.equal(_bits(v), before[k]), (what, k)

    N.check(lib.mvn_global_bias(dims, params, e.data_ptr(), B, gbias.data_ptr(), stream), "mvn_global_bias")
    d16 = N.make_dims(ls, ss, Q, 16, 16)
    touched = dict(fwd, out=out, gbias=gbias, ctx=ctx)
    before = snapshot(touched)
    for what, rc, code in (("C = 16", forward(d=d16), N.MVN_ERR_UNSUPPORTED),
                           ("context", forward(with_ctx=True), N.MVN_ERR_UNSUPPORTED),
                           ("gbias NULL", forward(gb=None), N.MVN_ERR_BAD_ARG)):
        assert rc == code, (what, rc, lib.mvn_last_error())
        unchanged(before, touched, "refused forward: " + what)
    inputs = dict(pd, index=index, e=e, gbias=gbias, ctx=ctx)
    before_in = snapshot(inputs)
    N.check(forward(), "mvn_forward_bf16_global")
    unchanged(before_in, inputs, "forward")
    assert bool(torch.isfinite(out).all())
    assert bool(torch.isnan(fwd["acts"][L]).all())  # (plane L is never written)

    # backward
    names = list(sd)
    grads = {k: g.new(tuple(sd[k].shape), 0.0, "grad " + k) for k in names}
    gp, _gkeep = ops.pack_params(dims, grads, L)
    gs = N.ParamGrads(gp.causal_w, gp.filter_w, gp.gate_w, gp.residual_w, gp.residual_b, gp.skip_w, gp.skip_b,
                      gp.head1_w, gp.head1_b, gp.head2_w, gp.head2_b, gp.ctx_filter_w, gp.ctx_filter_b,
                      gp.ctx_gate_w, gp.ctx_gate_b)
    bwd = dict(dx_a=g.new((B, C, Tp), NAN, "dx_a"), dx_b=g.new((B, C, Tp), NAN, "dx_b"),
               dfg=g.new((B, 2 * C, Tp), NAN, "dfg"), dskip=g.new((B, K, Sp), NAN, "dskip"),
               da1=g.new((B, Q, Sp), NAN, "da1"), dlogit=g.new((B, Q, Sp), NAN, "dlogit"))
    bb = N.BwdBuffers(*(bwd[k].data_ptr() for k in ("dx_a", "dx_b", "dfg", "dskip", "da1", "dlogit")), None)
    n_scratch = int(lib.mvn_global_bf16_scratch_floats(dims, B, T))
    scratch = g.new((n_scratch,), NAN, "scratch")
    rowsum = g.new((L, B, 128), NAN, "rowsum")
    dout = g.put(up.to(DEV), "dout")
    de = g.new((B, C), NAN, "de")

    def backward(d=dims, with_ctx=False, n=n_scratch, sc=scratch, rs=rowsum):
        return lib.mvn_backward_bf16_global(d, params, gs, index.data_ptr(), index.stride(0), B, T, fwd_struct(with_ctx),
                                            bb, out.data_ptr(), dout.data_ptr(), 0, 1,
                                            None if sc is None else sc.data_ptr(), n,
                                            None if rs is None else rs.data_ptr(), stream)

    touched = dict(bwd, scratch=scratch, rowsum=rowsum, **{"grad " + k: v for k, v in grads.items()})
    before = snapshot(touched)
    for what, rc, code in (("C = 16", backward(d=d16), N.MVN_ERR_UNSUPPORTED),
                           ("context", backward(with_ctx=True), N.MVN_ERR_UNSUPPORTED),
                           ("scratch one float short", backward(n=n_scratch - 1), N.MVN_ERR_BAD_ARG),
                           ("scratch NULL", backward(sc=None), N.MVN_ERR_BAD_ARG),
                           ("rowsum NULL", backward(rs=None), N.MVN_ERR_BAD_ARG)):
        assert rc == code, (what, rc, lib.mvn_last_error())
        unchanged(before, touched, "refused backward: " + what)
    saved = dict(inputs, out=out, dout=dout, **{k: v for k, v in fwd.items() if k != "z"})  # (z: the passes' scratch)
    before_in = snapshot(saved)
    N.check(backward(), "mvn_backward_bf16_global")
    assert lib.mvn_last_backward_form() == N.BWD_FORM_BF16_GLOBAL
    unchanged(before_in, saved, "backward")
    assert bool(torch.isfinite(rowsum).all())  # every (layer, sequence) row was written
    N.check(lib.mvn_global_bias_backward(dims, params, gs, rowsum.data_ptr(), e.data_ptr(), B, de.data_ptr(), stream),
            "mvn_global_bias_backward")
    g.check("mvn_global_bias_backward")
    last = f"residual_conv_stack.conv_layers.{L - 1}.conv_residual."
    for k in names:
        if k.startswith(last):  # never reaches the output: untouched
            assert float(grads[k].abs().max()) == 0.0, k
        else:
            assert torch.equal(grads[k], want[k]), k
    dE = torch.zeros(G, C, device=DEV).index_add_(0, feats.to(DEV), de)
    assert torch.allclose(dE, want["global_embedding.weight"], rtol=1e-6, atol=0.0)


# ---- 6. refusals in Python ------------------------------------------------------------------------------------------
def test_python_refusals():
    cfg = _cfg(2, 2, 64)
    full = make_state_dict(**cfg, seed=3)
    x = one_hot(synthetic_indices(2, 64, 64, 4), 64).to(DEV)
    feats = torch.tensor([0, 1]).to(DEV)
    video = torch.zeros(2, 1, 64, 64, 1, device=DEV)
    for precision in ("bf16", "fp32"):
        m = _model(cfg, full, _embedding(), precision=precision)
        with pytest.raises(ValueError, match="video context"):
            m(x, video, feats)
        with pytest.raises(ValueError, match="video context"):
            ops.wavenet_forward_loss(m, x, torch.zeros(2, 64, 64, device=DEV), gvec=torch.zeros(2, 64, device=DEV))
        assert m(x, None, feats).shape[0] == 2  # (the path exists without the video)
    cfg16 = _cfg(2, 2, 64, C=16)
    m16 = _model(cfg16, make_state_dict(**cfg16, seed=3), _embedding(16), precision="fp32")
    with pytest.raises(ValueError, match="residual_channels = skip_channels = 64"):
        m16(x, None, feats)
    m16.forward_precision = "bf16"
    with pytest.raises(ValueError, match="residual_channels = skip_channels = 64"):
        m16(x, None, feats)
    m = _model(cfg, full, _embedding(), path="auto")  # "auto" and "context" refuse labels under bf16 as before
    for path in ("auto", "context"):
        m.global_path = path
        with pytest.raises(ValueError, match="global"):
            m(x, None, feats)
    m.forward_precision = "fp16"
    m.global_path = "bias"
    with pytest.raises(ValueError, match="fp32' or 'bf16"):
        with torch.no_grad():
            m(x, None, feats)


# ---- 7. the trainer -----------------------------------------------------------------------------------------------
def test_trainer_bf16_with_labels(tmp_path, monkeypatch):
    import movenet_amd.wavenet as W
    from movenet_amd.config import arg_parser, config_from_args
    from movenet_amd.pytorch_lightning_trainer import Dance2Music, Trainer
    monkeypatch.setattr(W, "MAX_AUDIO_FRAMES", 2000)  # (the length every clip is resampled to)
    monkeypatch.setattr(W, "MAX_VIDEO_FRAMES", 2)
    rate, frames = 8000, 4000
    for split, per in (("train", 2), ("valid", 1)):
        for ci, context in enumerate(("salsa", "ballet")):
            d = tmp_path / "data" / split / context
            os.makedirs(d)
            for j in range(per):
                t = np.arange(frames) / rate
                y = 0.6 * np.sin(2 * np.pi * (220 + 110 * ci + 30 * j) * t) + 0.3 * np.sin(2 * np.pi * 50 * (j + 1) * t)
                with wave.open(str(d / f"c{j}.wav"), "wb") as w:
                    w.setnchannels(1)
                    w.setsampwidth(2)
                    w.setframerate(rate)
                    w.writeframes((y * 32767).round().astype("<i2").tobytes())
    out = tmp_path / "run"
    args = arg_parser().parse_args([
        "--dataset", str(tmp_path / "data"), "--use_video", "0", "--use_global", "1", "--global_dropout", "0.5",
        "--ema_decay", "0.9", "--precision", "bf16", "--input_channels", "64", "--residual_channels", "64",
        "--skip_channels", "64", "--layer_size", "4", "--stack_size", "2", "--batch_size", "2", "--val_batch_size", "2",
        "--n_epochs", "2", "--num_workers", "0", "--val_num_workers", "0", "--model_output_path", str(out)])
    module = Dance2Music(args.dataset, config_from_args(args))
    assert module.model.global_classes == 2 and module.model.global_path == "auto"
    before = {k: p.detach().clone() for k, p in module.model.named_parameters()}
    trainer = Trainer(max_epochs=2, default_root_dir=str(out), precision=args.precision)
    trainer.fit(module)
    assert module.model.forward_precision == "bf16" and module.model.global_path == "bias"
    assert N.lib().mvn_last_backward_form() == N.BWD_FORM_BF16_GLOBAL
    assert trainer.history and all(np.isfinite(r["train_loss"]) for r in trainer.history)
    after = dict(module.model.named_parameters())
    assert max((after[k].detach() - before[k].to(after[k].device)).abs().max().item() for k in before) > 1e-4
    moved = (after["global_embedding.weight"].detach().cpu() - before["global_embedding.weight"].cpu()).abs().max().item()
    assert moved > 0.0
    ckpts = sorted((out / "checkpoints").glob("*.ckpt"))
    ck = torch.load(ckpts[-1], map_location="cpu")
    assert ck["global_classes"] == ["ballet", "salsa"] and "ema_state_dict" in ck
    model = module.model.eval()
    model.generate_guidance = 2.0
    rf = model.receptive_fields
    prompt = one_hot(synthetic_indices(2, rf, 64, 77), 64).to(DEV)
    gen = model.generate(prompt, None, torch.tensor([1, 0]), n_samples=rf + 16, temperature=0.0)
    assert gen.shape == (2, 64, rf + 16)
