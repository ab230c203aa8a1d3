"""GPU: global conditioning on a class label (``WaveNet(global_classes=G)``).

A BUILD DEFINITION like the conditioned layer itself: the reference is this repository's oracle fed
``context = ctx + e[:, :, None]`` (e_b = E[class_b] or row_b @ E) and torch autograd on it.  Criteria of
test_conditioning_gpu.py: logits ``rel_err < 2e-5``, every gradient ``rel_err < 3e-4``.  Two paths are under test: the
fast one (C = K = 64, no video: one bias vector per layer and sequence, backward form MVN_BWD_FORM_ONE_GLOBAL) and the
general one (``global_path = "context"``: the existing conditioned kernels fed a constant context)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import one_hot, rel_err, synthetic_indices
from movenet_amd.utils.weights import make_state_dict
from oracle import wavenet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = 4
CLASSES = [2, 0, 2]  # a repeated class and (1, 3) absent ones


def _embedding(C, seed=99, classes=G):
    return torch.randn(classes, C, generator=torch.Generator().manual_seed(seed))


def _model(cfg, sd, E, **kw):
    from movenet_amd.wavenet import WaveNet
    m = WaveNet(**cfg, global_classes=E.shape[0], **kw)
    m.load_state_dict({**sd, "global_embedding.weight": E}, strict=True)
    return m.to(DEV)


def _cfg(layer_size, stack_size, Q, C=64):
    return dict(layer_size=layer_size, stack_size=stack_size, input_channels=Q, residual_channels=C, skip_channels=C)


def _oracle(cfg, sd, E, x, feats, kind, gout=None, dtype=torch.float32, ctx_of=None):
    """(value, {name: gradient}) of the oracle with context = ctx + e[:, :, None].  kind: "logits" (upstream gradient
    ``gout``), "reference" / "model" (the two loss rules).  ``ctx_of(params)`` -> the up-sampled video, or None."""
    dims = O.Dims(**cfg)
    params = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    Ep = E.to(dtype).clone().requires_grad_(True)
    e = Ep[feats] if not feats.is_floating_point() else feats.to(dtype) @ Ep
    ctx = e[:, :, None].expand(-1, -1, x.shape[2])
    if ctx_of is not None:
        ctx = ctx_of(params) + ctx
    xx = x.to(dtype)
    if kind == "logits":
        val = O.forward(params, dims, xx, context=ctx, output_unnormalized=False)
        (val * gout.to(dtype)).sum().backward()
    else:
        target = x[:, :, dims.receptive_fields:].argmax(1)
        out = O.forward(params, dims, xx, context=ctx, output_unnormalized=(kind == "reference"))
        val = F.cross_entropy(out, target)
        val.backward()
    grads = {k: p.grad for k, p in params.items() if p.grad is not None}
    grads["global_embedding.weight"] = Ep.grad
    return val.detach(), grads


def _device_run(m, x, feats, kind, gout=None, video=None):
    from movenet_amd import _native as N
    m.zero_grad(set_to_none=True)
    if kind == "logits":
        val = m(x.to(DEV), video, feats.to(DEV), output_unnormalized=False)
        (val * gout.to(DEV)).sum().backward()
    else:
        m.loss_rule = kind
        val, _, _ = m(x.to(DEV), video, feats.to(DEV), return_loss=True)
        val.backward()
    form = N.lib().mvn_last_backward_form()
    return val.detach().cpu(), {k: p.grad.cpu() for k, p in m.named_parameters() if p.grad is not None}, form


def _compare(val, grads, val_o, grads_o, what):
    worst = 0.0
    if val_o.dim():
        e = rel_err(val, val_o)
        print(f"{what}: logits rel_err {e:.2e}")
        assert e < 2e-5, (what, e)
    else:
        assert abs(val.item() - val_o.item()) < 2e-5 * max(abs(val_o.item()), 1e-30), (what, val.item(), val_o.item())
    want = grads_o
    assert sorted(grads) == sorted(want), what
    for k in want:
        e = rel_err(grads[k], want[k])
        worst = max(worst, e)
        assert e < 3e-4, (what, k, e)
    print(f"{what}: worst gradient rel_err {worst:.2e}")
    return worst


# ---- 1. the fast path at the training shapes -------------------------------------------------------------------
SHAPES = [(3, 2, 3, 300), (3, 2, 3, 17), (10, 1, 2, 1025), (10, 3, 1, 3170)]


@pytest.mark.parametrize("Q", [64, 256])
@pytest.mark.parametrize("layer_size,stack_size,B,T", SHAPES)
def test_fast_path_and_context_path_vs_oracle(monkeypatch, layer_size, stack_size, B, T, Q):
    """Both paths against the oracle under an upstream gradient on the logits and under both loss rules, then the fast
    path against float64: at most twice the general path's error, on the logits and on the worst gradient.  Both paths
    run the one-kernel layer backward (forms 5 and 3), so they share its rounding: measured worst gradient, fast /
    general, between 8.7e-7 / 8.3e-7 and 5.6e-6 / 5.1e-6 (the 30-layer case) over the eight cases."""
    from movenet_amd import _native as N
    monkeypatch.setenv("MOVENET_DEBUG_GUARD", "1")  # guard bands behind every scratch tensor of both passes
    cfg = _cfg(layer_size, stack_size, Q)
    dims = O.Dims(**cfg)
    if layer_size == 3 and T == 17:
        assert T == dims.receptive_fields + 1  # two head columns, one of them the output
    sd = make_state_dict(**cfg, seed=41, gain=1.5)
    sd = {k: v for k, v in sd.items() if not k.startswith("video_")}
    E = _embedding(64)
    feats = torch.tensor(CLASSES[:B])
    x = one_hot(synthetic_indices(B, T, Q, 1234), Q)
    S = T - dims.receptive_fields
    gout = torch.randn(B, Q, S, generator=torch.Generator().manual_seed(5))
    full = dict(make_state_dict(**cfg, seed=41, gain=1.5))
    m = _model(cfg, full, E).train()
    absent = [c for c in range(G) if c not in CLASSES[:B]]
    for kind in ("logits", "reference", "model"):
        val_o, grads_o = _oracle(cfg, sd, E, x, feats, kind, gout)
        for path in ("auto", "context"):
            m.global_path = path
            val, grads, got_form = _device_run(m, x, feats, kind, gout)
            print(f"{kind}/{path}: backward form {got_form}")
            if path == "auto":
                assert got_form == N.BWD_FORM_ONE_GLOBAL, got_form
            else:
                assert got_form == N.BWD_FORM_ONE, got_form
            _compare(val, grads, val_o, grads_o, f"{kind}/{path}")
            dE = grads["global_embedding.weight"]
            assert torch.equal(dE[absent], torch.zeros_like(dE[absent]))
    # the fast path against float64: at most twice the error of the general path (existing kernels fed a constant
    # context: the yardstick, not the code under test), on the logits and on the worst gradient
    val64, grads64 = _oracle(cfg, sd, E, x, feats, "logits", gout, dtype=torch.float64)
    err = {}
    for path in ("auto", "context"):
        m.global_path = path
        val, grads, _ = _device_run(m, x, feats, "logits", gout)
        per = {k: rel_err(grads[k].double(), grads64[k]) for k in grads64}
        worst = max(per, key=per.get)
        print(f"vs float64, {path}: worst gradient {worst} {per[worst]:.2e}")
        err[path] = (rel_err(val.double(), val64), per[worst])
    print(f"vs float64: fast logits {err['auto'][0]:.2e} gradients {err['auto'][1]:.2e}; "
          f"context logits {err['context'][0]:.2e} gradients {err['context'][1]:.2e}")
    assert err["auto"][0] <= 2 * err["context"][0], err
    assert err["auto"][1] <= 2 * err["context"][1], err


@pytest.mark.parametrize("Q", [64, 256])
@pytest.mark.parametrize("layer_size,stack_size,B,T", SHAPES)
def test_context_path_reports_form_one(layer_size, stack_size, B, T, Q):
    """``global_path = "context"`` reports MVN_BWD_FORM_ONE at every shape above: the conditioned layers' one-kernel
    form takes its second pair of gradient tensors and its slabs from the scratch ops.py hands mvn_backward_scratch --
    the (B, Q, Sp) dlogit / da1 tensors, where mvn_backward looks for that room, hold it at (3, 2, 3, 300), Q = 256
    alone of these shapes."""
    from movenet_amd import _native as N
    cfg = _cfg(layer_size, stack_size, Q)
    m = _model(cfg, make_state_dict(**cfg, seed=41, gain=1.5), _embedding(64)).train()
    m.global_path = "context"
    x = one_hot(synthetic_indices(B, T, Q, 1234), Q)
    gout = torch.randn(B, Q, T - O.Dims(**cfg).receptive_fields, generator=torch.Generator().manual_seed(5))
    _, _, form = _device_run(m, x, torch.tensor(CLASSES[:B]), "logits", gout)
    assert form == N.BWD_FORM_ONE, form


# ---- 2. a soft row ------------------------------------------------------------------------------------------
def test_soft_rows_vs_oracle():
    cfg = _cfg(3, 2, 64)
    full = make_state_dict(**cfg, seed=43, gain=1.5)
    sd = {k: v for k, v in full.items() if not k.startswith("video_")}
    E = _embedding(64)
    B, T = 3, 300
    rows = torch.softmax(torch.randn(B, G, generator=torch.Generator().manual_seed(3)), dim=1)
    x = one_hot(synthetic_indices(B, T, 64, 1234), 64)
    gout = torch.randn(B, 64, T - O.Dims(**cfg).receptive_fields, generator=torch.Generator().manual_seed(5))
    val_o, grads_o = _oracle(cfg, sd, E, x, rows, "logits", gout)
    m = _model(cfg, full, E).train()
    val, grads, _ = _device_run(m, x, rows, "logits", gout)
    _compare(val, grads, val_o, grads_o, "soft rows")


# ---- 3. label and video together ------------------------------------------------------------------------------
def test_label_and_video_together(monkeypatch):
    import movenet_amd.wavenet as W
    from movenet_amd import _native as N
    frames, B, cin = 7, 3, 3
    T = 1000 * frames
    monkeypatch.setattr(W, "MAX_AUDIO_FRAMES", T)
    monkeypatch.setattr(W, "MAX_VIDEO_FRAMES", frames)
    cfg = _cfg(3, 2, 256)
    sd = make_state_dict(**cfg, context_in_channels=cin, seed=29, gain=1.5)
    E = _embedding(64)
    feats = torch.tensor(CLASSES)
    x = one_hot(synthetic_indices(B, T, 256, 1234), 256)
    video = torch.from_numpy(np.random.default_rng(4321).random((B, frames, 64, 64, cin), dtype=np.float32))
    w = torch.linspace(0.5, 1.5, 256).view(1, 256, 1)
    m = _model(dict(cfg, context_in_channels=cin), sd, E).train()
    out = m(x.to(DEV), video.to(DEV), feats.to(DEV), output_unnormalized=False)
    (out * w.to(DEV)).square().mean().backward()
    assert N.lib().mvn_last_backward_form() == N.BWD_FORM_ONE
    got = {k: p.grad.cpu() for k, p in m.named_parameters() if p.grad is not None}

    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    Ep = E.clone().requires_grad_(True)
    ctx = O.upsample_video(params, video, expect_frames=T) + Ep[feats][:, :, None]
    out_o = O.forward(params, O.Dims(**cfg), x, context=ctx, output_unnormalized=False)
    (out_o * w).square().mean().backward()
    assert rel_err(out.detach().cpu(), out_o.detach()) < 2e-5
    want = {k: p.grad for k, p in params.items() if p.grad is not None}
    want["global_embedding.weight"] = Ep.grad
    assert sorted(got) == sorted(want)
    for k in want:
        assert rel_err(got[k], want[k]) < 3e-4, k


# ---- 4. other channel counts: the generic kernels ----------------------------------------------------------------
def test_small_channels_vs_oracle():
    from movenet_amd import _native as N
    cfg = _cfg(2, 2, 64, C=16)
    full = make_state_dict(**cfg, seed=17)
    sd = {k: v for k, v in full.items() if not k.startswith("video_")}
    E = _embedding(16)
    B, T = 3, 300
    feats = torch.tensor(CLASSES)
    x = one_hot(synthetic_indices(B, T, 64, 1234), 64)
    gout = torch.randn(B, 64, T - O.Dims(**cfg).receptive_fields, generator=torch.Generator().manual_seed(5))
    val_o, grads_o = _oracle(cfg, sd, E, x, feats, "logits", gout)
    m = _model(cfg, full, E).train()
    val, grads, form = _device_run(m, x, feats, "logits", gout)
    assert form == N.BWD_FORM_GENERIC
    _compare(val, grads, val_o, grads_o, "C = 16")


# ---- 5. generation -------------------------------------------------------------------------------------------
# (the dims of the existing conditioned generation tests: the small model, config 2, and the C = K = 128 model of
# test_conditioned_rounds_match_generic_kernel -- the only dims at which the fp16-operand PIPE_F16 kernel exists)
GEN_CFGS = [dict(layer_size=2, stack_size=2, input_channels=64, residual_channels=16, skip_channels=16),
            dict(layer_size=10, stack_size=3, input_channels=256, residual_channels=64, skip_channels=64),
            dict(layer_size=10, stack_size=6, input_channels=256, residual_channels=128, skip_channels=128)]
GEN_WANT = {16: "GENERIC", 64: "GENERIC STREAM PIPE FOLD", 128: "GENERIC PIPE PIPE_F16"}


@pytest.mark.parametrize("cfg", GEN_CFGS, ids=["small", "config2", "c128"])
def test_generators_take_a_global_context(cfg):
    """Every variant mvn_gen_variant grants (PIPE_F16, with its fp16-operand priming forward, among them):
    ``global_context=e`` gives the samples of the same kernels fed the expanded context, to the bit; on the small dims
    they are the oracle's cached generator's."""
    from movenet_amd import _native as N
    from movenet_amd.generation import GroupedGenerator, RingGenerator
    small = cfg["residual_channels"] == 16
    C, Q = cfg["residual_channels"], cfg["input_channels"]
    full = make_state_dict(**cfg, seed=3 if small else 1, gain=3.0 if small else 2.0 if C == 64 else 1.5, head_gain=6.0)
    sd = {k: v.to(DEV) for k, v in full.items() if not k.startswith("video_")}
    dims = O.Dims(**cfg)
    rf, B = dims.receptive_fields, 4
    n_total = rf + 64
    pidx = synthetic_indices(B, rf, Q, 77)
    e = 2.0 * _embedding(C, classes=B)
    lib = N.lib()
    variants = [v for v in (N.GEN_GENERIC, N.GEN_STREAM, N.GEN_PIPE, N.GEN_PIPE_F16, N.GEN_FOLD)
                if lib.mvn_gen_variant(N.make_dims(*[cfg[k] for k in ("layer_size", "stack_size", "input_channels",
                                                                      "residual_channels", "skip_channels")]), v, B) == v]
    # (what these dims are known to grant: a variant that silently dropped out would drop its case)
    assert variants == sorted(getattr(N, "GEN_" + name) for name in GEN_WANT[C].split()), variants

    def run(cls, variant, **kw):
        g = cls(**cfg, state_dict=sd, batch=B, n_total=n_total, device=DEV, variant=variant, temperature=0.0, **kw)
        g.prime(pidx.to(DEV))
        g.advance(64)
        g.check_errors()
        return g.samples.clone()

    want = None
    if small:
        ctx = e[:, :, None].expand(-1, -1, n_total).contiguous()
        want, _ = O.generate_ring({k: v.cpu() for k, v in sd.items()}, dims, pidx.numpy(), n_total, context=ctx.numpy())
        plain, _ = O.generate_ring({k: v.cpu() for k, v in sd.items()}, dims, pidx.numpy(), n_total)
        assert not np.array_equal(plain, want)  # the label matters
    for v in variants:
        by_vector = run(RingGenerator, v, global_context=e.to(DEV))
        by_tensor = run(RingGenerator, v, context=e.to(DEV)[:, :, None].expand(-1, -1, n_total))
        assert torch.equal(by_vector, by_tensor), v
        if want is not None:
            assert np.array_equal(by_vector.cpu().numpy(), want), v
    pipelined = [v for v in variants if v in (N.GEN_FOLD, N.GEN_PIPE)]
    assert bool(pipelined) == (not small)  # (the small dims have no pipelined kernel to group)
    if pipelined:
        single = run(RingGenerator, pipelined[0], global_context=e.to(DEV))
        grouped = run(GroupedGenerator, pipelined[0], group=2, global_context=e.to(DEV))
        assert torch.equal(single, grouped)


def test_generate_end_to_end_follows_the_label():
    cfg = GEN_CFGS[0]
    full = make_state_dict(**cfg, seed=3, gain=1.5, head_gain=6.0)
    E = 3.0 * _embedding(16)
    assert not torch.equal(E[0], E[1])
    m = _model(cfg, full, E)
    rf = m.receptive_fields
    prompt = one_hot(synthetic_indices(1, rf, 64, 77), 64).repeat(2, 1, 1).to(DEV)
    out = m.generate(prompt, None, torch.tensor([0, 1]), n_samples=rf + 64, temperature=0.0)
    assert out.shape == (2, 64, rf + 64)
    assert torch.equal(out[0, :, :rf], out[1, :, :rf]) and not torch.equal(out[0], out[1])
    sd = {k: v for k, v in full.items() if not k.startswith("video_")}
    ctx = E[:2][:, :, None].expand(-1, -1, rf + 64).contiguous()
    want, _ = O.generate_ring(sd, O.Dims(**cfg), prompt.argmax(1).cpu().numpy(), rf + 64, context=ctx.numpy())
    assert np.array_equal(out.argmax(1).cpu().numpy(), want)


# ---- 6. refusals -----------------------------------------------------------------------------------------------
def test_refusals():
    cfg = _cfg(3, 2, 64)
    m = _model(cfg, make_state_dict(**cfg, seed=1), _embedding(64))
    x = one_hot(synthetic_indices(2, 100, 64, 1), 64).to(DEV)
    ok = torch.tensor([0, 1])
    with pytest.raises(ValueError, match="global_features"):
        m(x)
    with pytest.raises(ValueError, match="global_features"):
        m.generate(x)
    for bad in (torch.tensor([0, 1, 2]), torch.tensor([0, G]), torch.tensor([-1, 0]), torch.rand(2, G + 1),
                torch.rand(3, G)):
        with pytest.raises(ValueError):
            m(x, None, bad)
        with pytest.raises(ValueError):
            m.generate(x, None, bad)
    m.forward_precision = "bf16"
    with pytest.raises(ValueError, match="global"):
        m(x, None, ok)
    m.forward_precision = "fp32"
    assert m(x, None, ok).shape[0] == 2
    with pytest.raises(ValueError):
        m.global_path = "fast"


# ---- 7. trainer ------------------------------------------------------------------------------------------------
def test_trainer_with_use_global(tmp_path, monkeypatch):
    import os
    import wave
    import movenet_amd.wavenet as W
    from movenet_amd.checkpoint import load_into
    from movenet_amd.config import arg_parser, config_from_args
    from movenet_amd.pytorch_lightning_trainer import Dance2Music, Trainer
    from movenet_amd.wavenet import WaveNet
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
        "--dataset", str(tmp_path / "data"), "--use_video", "0", "--use_global", "1", "--input_channels", "64",
        "--residual_channels", "64", "--skip_channels", "64", "--layer_size", "4", "--stack_size", "2",
        "--batch_size", "2", "--val_batch_size", "2", "--n_epochs", "2",
        "--num_workers", "0", "--val_num_workers", "0", "--model_output_path", str(out)])
    module = Dance2Music(args.dataset, config_from_args(args))
    assert module.global_classes == ["ballet", "salsa"] and module.model.global_classes == 2
    before = module.model.global_embedding.weight.detach().clone()
    trainer = Trainer(max_epochs=2, default_root_dir=str(out))
    trainer.fit(module)
    assert trainer.history and all(np.isfinite(r["train_loss"]) for r in trainer.history)
    ckpts = sorted((out / "checkpoints").glob("*.ckpt"))
    ck = torch.load(ckpts[-1], map_location="cpu")
    assert ck["global_classes"] == ["ballet", "salsa"]
    trained = ck["state_dict"]["model.global_embedding.weight"]
    assert trained.shape == (2, 64)
    moved = (trained - before.cpu()).abs().amax(1)
    assert bool((moved > 0).all())  # both classes were seen
    # a reloaded model reproduces the TRAINED one's logits to the bit
    reloaded = WaveNet(4, 2, 64, 64, 64, global_classes=2)
    load_into(reloaded, ckpts[-1])
    x = one_hot(synthetic_indices(2, 200, 64, 9), 64).to(DEV)
    cls = torch.tensor([1, 0])
    with torch.no_grad():
        want = module.model.eval()(x, None, cls, output_unnormalized=False)
        got = reloaded.to(DEV).eval()(x, None, cls, output_unnormalized=False)
    assert torch.equal(got, want)
    assert not torch.equal(want, module.model(x, None, torch.tensor([0, 0]), output_unnormalized=False).detach())
