"""GPU: video-conditioned training in bf16 -- ``WaveNet.bf16_context`` under ``forward_precision = "bf16"`` (DESIGN 4.3d;
mvn_forward_bf16_ctx / mvn_backward_bf16_ctx, backward form MVN_BWD_FORM_BF16_CTX).

Forward the context is a third K block of the f | g contraction on bf16 operands, the accumulators started from the fp32
bcf | bcg; backward the layer kernel's arithmetic is the audio-only mode's, its fp32 df | dg tile goes to the dfg tensor
and the fp32 context pass forms dctx, dWc, dbc from unrounded operands.  Yardsticks: the fp32 oracle with a context and
tests/bf16_ctx_emulation.py.  Criteria (test_bf16_train_gpu.py's), applied to every parameter, the four context tensors
of every layer and the gradient of the context itself:
  logits      rel_err(got, oracle) <= 2 x rel_err(emulation, oracle)
  gradients   cosine with the oracle's >= min(0.99, the emulation's worst - 0.005);
              norm within max(3 %, 1.5 x the emulation's worst norm deviation) of the oracle's

Shapes (layers, stacks, Q, B, T):
  a  2 x 2, 256, 2, 300     b  2 x 2, 64, 16, 1100     c  10 x 1, 64, 2, 1025 (last dilation past the valid span)
  d  10 x 3, 256, 2, 3073 (T = RF + 1)                 e  10 x 3, 256, 3, 3170
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bf16_ctx_emulation as EC
from helpers import _Guard, one_hot, rel_err, synthetic_indices
from movenet_amd import _native as N
from movenet_amd import ops
from movenet_amd.utils.weights import make_state_dict
from oracle import wavenet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = {"a": (2, 2, 256, 2, 300), "b": (2, 2, 64, 16, 1100), "c": (10, 1, 64, 2, 1025), "d": (10, 3, 256, 2, 3073),
          "e": (10, 3, 256, 3, 3170)}
NAN = float("nan")
CTX = "context"  # the key the gradient of the context is filed under


def _model(cfg, full, precision="bf16", context=True, **kw):
    from movenet_amd.wavenet import WaveNet
    m = WaveNet(**cfg, **kw)
    m.load_state_dict(dict(full), strict=False)
    m.forward_precision = precision
    m.bf16_context = context
    return m.to(DEV)


@functools.lru_cache(maxsize=None)
def _case(name, seed=7):
    ls, ss, Q, B, T = SHAPES[name]
    cfg = dict(layer_size=ls, stack_size=ss, input_channels=Q, residual_channels=64, skip_channels=64)
    full = make_state_dict(**cfg, seed=seed)
    sd = {k: v for k, v in full.items() if not k.startswith("video_")}
    dims = O.Dims(**cfg)
    assert T >= dims.receptive_fields + 1
    x = one_hot(synthetic_indices(B, T, Q, seed + 1), Q)
    ctx = torch.randn(B, 64, T, generator=torch.Generator().manual_seed(seed + 2))
    up = torch.randn(B, Q, T - dims.receptive_fields, generator=torch.Generator().manual_seed(11))
    return cfg, dims, full, sd, x, ctx, up


def _cos(a, b) -> float:
    a, b = a.double().flatten(), b.double().flatten()
    return (a @ b / (a.norm() * b.norm()).clamp_min(1e-300)).item()


def _norm_dev(a, ref) -> float:
    return abs(a.double().norm().item() - ref.double().norm().item()) / ref.double().norm().item()


def _check_grads(got, oracle, emu, what):
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


def _reference(sd, dims, x, ctx, kind, up, logits_fn, extra=None):
    """(logits, {name: gradient}) of ``logits_fn(params, context)``; the context's gradient is filed under CTX.
    ``extra``: {name: leaf} -> the context is ``ctx + f(extra)`` (test 5), the leaves' gradients filed under their names."""
    params = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    c = ctx.clone().requires_grad_(True)
    leaves = {k: v.clone().requires_grad_(True) for k, v in (extra or {}).items()}
    cc = c if not leaves else c + leaves["global_embedding.weight"][extra_rows(c.shape[0])][:, :, None]
    lg = logits_fn(params, cc)[:, :, :-1]
    if kind == "loss":
        target = x[:, :, dims.receptive_fields:].argmax(1)
        F.cross_entropy(F.softmax(lg, dim=1), target).backward()
    else:
        (lg * up).sum().backward()
    grads = {k: p.grad for k, p in params.items() if p.grad is not None}
    grads[CTX] = c.grad
    for k, v in leaves.items():
        grads[k] = v.grad
    return lg.detach(), grads


CLASSES = [2, 2, 0, 1, 3, 0, 2, 1, 1, 3, 0, 0, 2, 3, 1, 2]


def extra_rows(batch):
    return torch.tensor(CLASSES[:batch])


@functools.lru_cache(maxsize=None)
def _refs(name, kind):
    cfg, dims, full, sd, x, ctx, up = _case(name)
    ref = _reference(sd, dims, x, ctx, kind, up, lambda p, c: O.logits_full(p, dims, x, context=c))
    emu = _reference(sd, dims, x, ctx, kind, up, lambda p, c: EC.logits(p, dims, x, c))
    return ref, emu


def _device_step(m, x, ctx, kind, up, gvec_of=None):
    """One step through ops with the context as a leaf: (logits or None, {name: gradient}, backward form)."""
    m.zero_grad(set_to_none=True)
    c = None if ctx is None else ctx.to(DEV).requires_grad_(True)
    gvec = None if gvec_of is None else gvec_of(m)
    if kind == "loss":
        loss, _acc, _probs = ops.wavenet_forward_loss(m, x.to(DEV), c, gvec=gvec)
        loss.backward()
        out = None
    else:
        out = ops.wavenet_forward(m, x.to(DEV), c, output_unnormalized=False, gvec=gvec)
        (out * up.to(DEV)).sum().backward()
        out = out.detach().cpu()
    form = N.lib().mvn_last_backward_form()
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
    if c is not None:
        grads[CTX] = c.grad.detach().clone()
    return out, grads, form


# ---- 1. zero context weights are the audio-only model, to the bit ----------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_zero_context_weights_equal_audio_only_to_the_bit(name):
    """Zero context-conv weights and biases, a random finite context: the conditioned kernels must give the audio-only
    kernels' bits in the logits and in every non-context gradient (torch.equal) -- everything in them but the third K
    block, the bias start and the dfg store; the layer pass cuts each sequence into the same chunks (sequence.hip).  The
    context-conv gradients, sum dfg ctx^T and sum dfg, are non-zero; dctx = Wc^T dfg is zero."""
    cfg, dims, full, sd, x, ctx, up = _case(name)
    zeroed = {k: (torch.zeros_like(v) if "context_conv" in k else v) for k, v in full.items()}
    video, plain = _model(cfg, zeroed).train(), _model(cfg, zeroed, context=False).train()
    for kind in ("loss", "logits"):
        out_v, g_v, form_v = _device_step(video, x, ctx, kind, up)
        assert form_v == N.BWD_FORM_BF16_CTX, form_v
        out_p, g_p, form_p = _device_step(plain, x, None, kind, up)
        assert form_p == N.BWD_FORM_BF16, form_p
        if kind == "logits":
            assert torch.equal(out_v, out_p)
        assert g_p and not any("context_conv" in k for k in g_p)
        for k, g in g_p.items():
            assert torch.equal(g_v[k], g), (kind, k)
        cw = [k for k in g_v if "context_conv" in k]
        assert len(cw) == 4 * dims.n_layers
        for k in cw:
            assert bool(torch.isfinite(g_v[k]).all()) and float(g_v[k].abs().max()) > 0.0, (kind, k)
        assert float(g_v[CTX].abs().max()) == 0.0


# ---- 2. against the oracle with a context, calibrated on the emulation ------------------------------------------------
@pytest.mark.parametrize("kind", ["loss", "logits"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_against_oracle_and_emulation(monkeypatch, name, kind):
    monkeypatch.setenv("MOVENET_DEBUG_GUARD", "1")  # guard bands behind every scratch tensor of both passes
    cfg, dims, full, sd, x, ctx, up = _case(name)
    (lg_ref, g_ref), (lg_emu, g_emu) = _refs(name, kind)
    m = _model(cfg, full).train()
    out, got, form = _device_step(m, x, ctx, kind, up)
    assert form == N.BWD_FORM_BF16_CTX, form
    if out is not None:
        e_got, e_emu = rel_err(out, lg_ref), rel_err(lg_emu, lg_ref)
        print(f"{name}/{kind}: logits rel. err bf16 HIP {e_got:.2e}, emulation {e_emu:.2e}")
        assert e_got <= 2 * e_emu, (e_got, e_emu)
        with torch.no_grad():
            exact = ops.wavenet_forward(_model(cfg, full, "fp32"), x.to(DEV), ctx.to(DEV), output_unnormalized=False).cpu()
        assert not torch.equal(out, exact)  # the bf16 kernels ran
    assert sum("context_conv" in k for k in got) == 4 * dims.n_layers and CTX in got
    _check_grads(got, g_ref, g_emu, f"{name}/{kind}")


# ---- 3. + 4. the C ABI: padding and poison, refusals that launch nothing -------------------------------------------
def _bits(t):
    return t.detach().reshape(-1).view(torch.int32).clone()


def test_c_abi_padding_poison_and_refusals():
    """Shape (a) through ctypes, every buffer NaN-filled between sentinel bands.  Refused calls (C = 16; no ctx, dctx or
    dfg; ctx_ld < T; a scratch one float short) return the documented code, agree with mvn_bf16_ctx_path and leave every
    buffer's bits alone.  Then the same step twice: ctx_ld = Tp + 37 with NaN in every context column outside [0, T) and
    dfg / dctx pre-filled with NaN, against a tight ctx_ld = T copy -- logits and every gradient equal bit for bit, and
    all are finite."""
    lib = N.lib()
    cfg, dims_o, full, sd, x, ctx_h, up = _case("a")
    ls, ss, Q, B, T = SHAPES["a"]
    C = K = 64
    L, S = dims_o.n_layers, T - dims_o.receptive_fields + 1
    stream = torch.cuda.current_stream(DEV).cuda_stream
    g = _Guard(front=True)
    dims, d16 = N.make_dims(ls, ss, Q, C, K), N.make_dims(ls, ss, Q, 16, 16)
    Tp, Sp = lib.mvn_padded_len(T), lib.mvn_padded_len(S + 31)
    pd = {k: g.put(v.to(DEV), k) for k, v in sd.items()}
    params, _keep = ops.pack_params(dims, pd, L)
    index = g.put(x.argmax(1).to(DEV, torch.int32), "index")
    fwd = dict(acts=g.new((L + 1, B, C, Tp), NAN, "acts"), th=g.new((L, B, C, Tp), NAN, "th"),
               sg=g.new((L, B, C, Tp), NAN, "sg"), z=g.new((B, C, Tp), NAN, "z"), skip=g.new((B, K, Sp), NAN, "skip"),
               a1=g.new((B, Q, Sp), NAN, "a1"))
    out = g.new((B, Q, S - 1), NAN, "out")
    wide_ld = Tp + 37
    ctx_wide = g.new((B, C, wide_ld), NAN, "ctx wide")
    ctx_wide[:, :, :T] = ctx_h.to(DEV)
    ctx_tight = g.put(ctx_h.to(DEV), "ctx tight")
    grads = {k: g.new(tuple(sd[k].shape), 0.0, "grad " + k) for k in sd}
    gp, _gkeep = ops.pack_params(dims, grads, L)
    gs = N.ParamGrads(gp.causal_w, gp.filter_w, gp.gate_w, gp.residual_w, gp.residual_b, gp.skip_w, gp.skip_b,
                      gp.head1_w, gp.head1_b, gp.head2_w, gp.head2_b, gp.ctx_filter_w, gp.ctx_filter_b,
                      gp.ctx_gate_w, gp.ctx_gate_b)
    bwd = dict(dx_a=g.new((B, C, Tp), NAN, "dx_a"), dx_b=g.new((B, C, Tp), NAN, "dx_b"),
               dfg=g.new((B, 2 * C, Tp), NAN, "dfg"), dskip=g.new((B, K, Sp), NAN, "dskip"),
               da1=g.new((B, Q, Sp), NAN, "da1"), dlogit=g.new((B, Q, Sp), NAN, "dlogit"),
               dctx=g.new((B, C, Tp), NAN, "dctx"))
    n_scratch = int(lib.mvn_bf16_ctx_scratch_floats(dims, B, T))
    scratch = g.new((n_scratch,), NAN, "scratch")
    dout = g.put(up.to(DEV), "dout")

    def fwd_struct(c, ld):
        return N.FwdBuffers(fwd["acts"].data_ptr(), fwd["th"].data_ptr(), fwd["sg"].data_ptr(), fwd["z"].data_ptr(),
                            fwd["skip"].data_ptr(), fwd["a1"].data_ptr(), None if c is None else c.data_ptr(), ld, None, 0)

    def forward(d=dims, c=ctx_wide, ld=wide_ld):
        return lib.mvn_forward_bf16_ctx(d, params, index.data_ptr(), index.stride(0), B, T, fwd_struct(c, ld),
                                        out.data_ptr(), 0, 1, 1, stream)

    def backward(d=dims, c=ctx_wide, ld=wide_ld, drop=(), n=n_scratch):
        bb = N.BwdBuffers(*(None if k in drop else bwd[k].data_ptr()
                            for k in ("dx_a", "dx_b", "dfg", "dskip", "da1", "dlogit", "dctx")))
        return lib.mvn_backward_bf16_ctx(d, params, gs, index.data_ptr(), index.stride(0), B, T, fwd_struct(c, ld), bb,
                                         out.data_ptr(), dout.data_ptr(), 0, 1, scratch.data_ptr(), n, stream)

    def snapshot(tensors):
        torch.cuda.synchronize()
        return {k: _bits(v) for k, v in tensors.items()}

    def unchanged(before, tensors, what):
        g.check(what)
        for k, v in tensors.items():
            assert torch.equal(_bits(v), before[k]), (what, k)

    assert lib.mvn_bf16_ctx_path(dims, B, T) == 1 and lib.mvn_bf16_ctx_path(d16, B, T) == 0
    everything = dict(fwd, out=out, scratch=scratch, **bwd, **{"grad " + k: v for k, v in grads.items()})
    before = snapshot(everything)
    UNS, BAD = N.MVN_ERR_UNSUPPORTED, N.MVN_ERR_BAD_ARG
    for what, call, code in (("fwd C = 16", lambda: forward(d=d16), UNS), ("fwd no ctx", lambda: forward(c=None, ld=0), BAD),
                             ("fwd ctx_ld < T", lambda: forward(ld=T - 1), BAD),
                             ("bwd C = 16", lambda: backward(d=d16), UNS), ("bwd no ctx", lambda: backward(c=None, ld=0), BAD),
                             ("bwd no dctx", lambda: backward(drop=("dctx",)), BAD),
                             ("bwd no dfg", lambda: backward(drop=("dfg",)), BAD),
                             ("bwd ctx_ld < T", lambda: backward(ld=T - 1), BAD),
                             ("bwd scratch one float short", lambda: backward(n=n_scratch - 1), BAD)):
        rc = call()
        assert rc == code, (what, rc, lib.mvn_last_error())
        # (the path query answers 0 exactly where the entry points answer MVN_ERR_UNSUPPORTED)
        assert (lib.mvn_bf16_ctx_path(d16 if "C = 16" in what else dims, B, T) == 0) == (code == UNS), what
        unchanged(before, everything, "refused: " + what)

    def step(c, ld):
        for v in grads.values():
            v.zero_()
        for k in ("dfg", "dctx"):
            bwd[k].fill_(NAN)
        N.check(forward(c=c, ld=ld), "mvn_forward_bf16_ctx")
        logits = out.clone()
        N.check(backward(c=c, ld=ld), "mvn_backward_bf16_ctx")
        assert lib.mvn_last_backward_form() == N.BWD_FORM_BF16_CTX
        g.check("step")
        return logits, {k: v.clone() for k, v in grads.items()}, bwd["dctx"][:, :, :T].clone()

    inputs = dict(pd, index=index, ctx_wide=ctx_wide, ctx_tight=ctx_tight, dout=dout)
    before_in = snapshot(inputs)
    lg_w, gr_w, dc_w = step(ctx_wide, wide_ld)
    lg_t, gr_t, dc_t = step(ctx_tight, T)
    unchanged(before_in, inputs, "inputs")
    assert bool(torch.isfinite(lg_w).all()) and torch.equal(lg_w, lg_t)
    assert bool(torch.isfinite(dc_w).all()) and torch.equal(dc_w, dc_t) and float(dc_w.abs().max()) > 0.0
    assert float(bwd["dctx"][:, :, T:].abs().max()) == 0.0  # (written in full: columns >= t_len are zero)
    last = f"residual_conv_stack.conv_layers.{L - 1}.conv_residual."
    for k in sd:
        assert bool(torch.isfinite(gr_w[k]).all()) and torch.equal(gr_w[k], gr_t[k]), k
        assert k.startswith(last) or float(gr_w[k].abs().max()) > 0.0, k
    # and they are the module's step
    m = _model(cfg, full).train()
    out_m, want, form = _device_step(m, x, ctx_h, "logits", up)
    assert form == N.BWD_FORM_BF16_CTX and torch.equal(out_m, lg_w.cpu())
    for k in sd:
        if not k.startswith(last):
            assert torch.equal(gr_w[k], want[k]), k
    assert torch.equal(dc_w, want[CTX])


# ---- 5. labels and video ------------------------------------------------------------------------------------------
def test_labels_ride_in_the_context():
    """global_classes = 4 with global_path "auto": the label's vector joins the context, so logits and parameter
    gradients are those of the unlabelled model fed ``context + e[:, :, None]``, bit for bit; the embedding's gradient
    meets the criteria of test 2 against the oracle.  "bias" with video keeps raising."""
    cfg, dims, full, sd, x, ctx, up = _case("a")
    B = x.shape[0]
    E = torch.randn(4, 64, generator=torch.Generator().manual_seed(99))
    feats = extra_rows(B)
    labelled = _model(cfg, {**full, "global_embedding.weight": E}, global_classes=4).train()
    assert labelled.global_path == "auto"
    plain = _model(cfg, full).train()
    e = E[feats]
    out_l, g_l, form_l = _device_step(labelled, x, ctx, "logits", up, gvec_of=lambda m: m.global_embedding.weight[feats.to(DEV)])
    out_p, g_p, form_p = _device_step(plain, x, ctx + e[:, :, None], "logits", up)
    assert form_l == form_p == N.BWD_FORM_BF16_CTX
    assert torch.equal(out_l, out_p)
    for k in g_p:
        if k != CTX:
            assert torch.equal(g_l[k], g_p[k]), k
    ref = _reference(sd, dims, x, ctx, "logits", up, lambda p, c: O.logits_full(p, dims, x, context=c),
                     extra={"global_embedding.weight": E})
    emu = _reference(sd, dims, x, ctx, "logits", up, lambda p, c: EC.logits(p, dims, x, c),
                     extra={"global_embedding.weight": E})
    key = "global_embedding.weight"
    _check_grads({key: g_l[key]}, {key: ref[1][key]}, {key: emu[1][key]}, "labels + video: dE")
    labelled.global_path = "bias"
    with pytest.raises(ValueError, match="video context"):
        _device_step(labelled, x, ctx, "logits", up, gvec_of=lambda m: m.global_embedding.weight[feats.to(DEV)])
    labelled.global_path = "auto"
    labelled.bf16_context = False
    with pytest.raises(ValueError, match="no video context"):
        _device_step(labelled, x, ctx, "logits", up, gvec_of=lambda m: m.global_embedding.weight[feats.to(DEV)])


# ---- 6. the trainer -----------------------------------------------------------------------------------------------
def test_trainer_bf16_video_fit(tmp_path, monkeypatch):
    import movenet_amd.wavenet as W
    from movenet_amd.config import ModelConfig, TrainingConfig
    from movenet_amd.pytorch_lightning_trainer import Dance2Music, Trainer
    mc = ModelConfig(layer_size=2, stack_size=2, input_channels=64, residual_channels=64, skip_channels=64)
    cfg = TrainingConfig(model_config=mc, batch_size=1, val_batch_size=1, n_epochs=1, use_video=True, optimizer="AdamW",
                         learning_rate=1e-3, model_output_path=tmp_path / "run", gradient_clipping=0.0)
    # (video batches need frames % 1000 == 0, and the clip length is a module constant, as in the reference: one video
    # frame <-> 1000 samples)
    monkeypatch.setattr(W, "MAX_AUDIO_FRAMES", 1000)
    monkeypatch.setattr(W, "MAX_VIDEO_FRAMES", 1)
    spec = "synthetic://clips=2,frames=1000"
    with pytest.raises(ValueError, match="audio-only"):
        Trainer(max_epochs=1, default_root_dir=tmp_path / "no", precision="bf16").fit(Dance2Music(spec, cfg))
    m = Dance2Music(spec, cfg)
    tr = Trainer(max_epochs=1, default_root_dir=tmp_path / "run", precision="bf16", bf16_video=True)
    tr.fit(m)
    assert m.model.forward_precision == "bf16" and m.model.bf16_context is True
    assert N.lib().mvn_last_backward_form() == N.BWD_FORM_BF16_CTX
    losses = [h["train_loss"] for h in tr.history]
    assert len(losses) == 2 and np.isfinite(losses).all()
