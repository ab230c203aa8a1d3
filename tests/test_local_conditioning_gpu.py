"""GPU: WaveNet(local_channels=M, local_hop=hop) end to end -- Q = 64, C = K = 32, 2 x 2 layers, M = 8, hop 16,
T = RF + 40 -- against the oracle fed the float64-made context (tests/logmel_reference.upsample_features).

Bounds: logits 2e-5 and gradients 3e-4 relative to the tensor's maximum, the video-context parity test's
(tests/test_conditioning_gpu.py); bf16 against fp32 as tests/test_bf16_video_gpu.py bounds its logits, by twice the
error of its bf16 emulation (tests/bf16_ctx_emulation.py) on the same data."""
import functools
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import logmel_reference as R
from helpers import DEV, one_hot, rel_err, synthetic_indices
from movenet_amd import ops
from movenet_amd.generation import RingGenerator, auto_plan
from movenet_amd.utils.weights import make_state_dict
from oracle import wavenet_oracle as O

pytestmark = pytest.mark.gpu
M, HOP, B = 8, 16, 2


def _cfg(C=32):
    return dict(layer_size=2, stack_size=2, input_channels=64, residual_channels=C, skip_channels=C)


@functools.lru_cache(maxsize=None)
def _case(C=32, gain=1.0, extra=40):
    cfg = _cfg(C)
    sd = make_state_dict(**cfg, seed=23, gain=gain, **({"head_gain": 6.0} if gain != 1.0 else {}))
    g = torch.Generator().manual_seed(5)
    sd["local_conv.weight"] = torch.randn(C, M, 1, generator=g) / M ** 0.5
    sd["local_conv.bias"] = 0.3 * torch.randn(C, generator=g)
    dims = O.Dims(**cfg)
    T = dims.receptive_fields + extra
    idx = synthetic_indices(B, T, 64, 77)
    feats = torch.randn(B, M, (T - 1) // HOP + 1, generator=g)
    return cfg, sd, dims, T, idx, feats


def _model(C=32, gain=1.0, **kw):
    from movenet_amd.wavenet import WaveNet
    cfg, sd = _case(C, gain)[:2]
    m = WaveNet(**cfg, local_channels=M, local_hop=HOP, **kw)
    missing = m.load_state_dict(sd, strict=False)
    assert [k for k in missing.missing_keys if not k.startswith("global_embedding")] == [] and not missing.unexpected_keys
    return m.to(DEV)


def _context64(sd, feats, T, leaves=None):
    w = sd["local_conv.weight"][:, :, 0].double() if leaves is None else leaves[0][:, :, 0]
    b = sd["local_conv.bias"].double() if leaves is None else leaves[1]
    return R.upsample_features(feats.double(), w, b, HOP, T)


def test_forward_is_the_context_path_to_the_bit_and_matches_the_oracle():
    cfg, sd, dims, T, idx, feats = _case()
    m = _model().eval()
    x = one_hot(idx, 64).to(DEV)
    f = feats.to(DEV)
    with torch.no_grad():
        ctx = ops.upsample_features(m, f, T)
        assert tuple(ctx.shape) == (B, 32, T)
        assert rel_err(ctx.cpu(), _context64(sd, feats, T)) < 1e-5
        got = m(x, local_features=f, output_unnormalized=False)
        assert torch.equal(got, ops.wavenet_forward(m, x, context=ctx, output_unnormalized=False))
        want = O.forward({k: v for k, v in sd.items() if not k.startswith("local_conv")}, dims, one_hot(idx, 64),
                         context=_context64(sd, feats, T).float(), output_unnormalized=False)
    assert rel_err(got.cpu(), want) < 2e-5
    plain = ops.wavenet_forward(m, x, context=torch.zeros_like(ctx), output_unnormalized=False)
    assert not torch.equal(got, plain)   # the features matter


def test_fused_loss_gradients_match_oracle_autograd():
    cfg, sd, dims, T, idx, feats = _case()
    x = one_hot(idx, 64)
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items() if not k.startswith("local_conv")}
    leaves = [sd["local_conv.weight"].double().requires_grad_(True), sd["local_conv.bias"].double().requires_grad_(True)]
    out_o = O.forward(params, dims, x, context=_context64(sd, feats, T, leaves).float())
    target = x[:, :, dims.receptive_fields:].argmax(1)
    loss_o = F.cross_entropy(out_o, target)
    loss_o.backward()
    m = _model().train()
    loss, _acc, _probs = m(x.to(DEV), return_loss=True, local_features=feats.to(DEV))
    loss.backward()
    assert abs(loss.item() - loss_o.item()) < 2e-6
    assert rel_err(m.local_conv.weight.grad.cpu(), leaves[0].grad) < 3e-4
    assert rel_err(m.local_conv.bias.grad.cpu(), leaves[1].grad) < 3e-4
    got = dict(m.named_parameters())
    for k in ("residual_conv_stack.conv_layers.1.context_conv_gate.weight", "causal_conv.conv.weight"):
        assert rel_err(got[k].grad.cpu(), params[k].grad) < 3e-4, k


def test_lengths_are_accepted_and_mask_the_loss():
    cfg, sd, dims, T, idx, feats = _case()
    rf = dims.receptive_fields
    lengths = [T, 15]   # sequence 1: 15 real samples of 48, so frame 2 (columns 16 on) touches padding only
    x = one_hot(idx, 64).to(DEV)
    f = feats.to(DEV).requires_grad_(True)
    m = _model().train()
    loss, _acc, probs = m(x, return_loss=True, lengths=lengths, local_features=f)
    loss.backward()
    valid = ops.valid_columns(lengths, T, rf)
    with torch.no_grad():   # the masked loss of the same call, from its own probabilities
        target = idx[:, rf:].to(DEV)
        per = F.cross_entropy(probs, target, reduction="none")
        mask = torch.arange(per.shape[1], device=DEV)[None, :] < torch.tensor(valid, device=DEV)[:, None]
        want = (per * mask).sum() / sum(valid)
    assert abs(loss.item() - want.item()) < 2e-6
    # gradient 0 in the padded columns: features whose every column lies in the padding receive exactly 0
    cut = lengths[1]   # columns >= cut of sequence 1 are padding; frame j reaches the columns (j - 1) hop .. (j + 1) hop
    first_dead = (cut + HOP - 1) // HOP + 1
    assert first_dead == 2 and f.shape[2] == 3   # the shape makes the check below run
    assert bool((f.grad[1, :, first_dead:] == 0).all()), "a frame that touches only padded columns received a gradient"
    assert float(f.grad[1, :, :first_dead].abs().max()) > 0 and float(f.grad[0, :, first_dead:].abs().max()) > 0
    # ... and at the context itself: the same loss on the up-sampled tensor as a leaf of its own
    m.zero_grad(set_to_none=True)
    ctx = ops.upsample_features(m, feats.to(DEV), T).detach().requires_grad_(True)
    loss2, _, _ = ops.wavenet_forward_loss(m, x, ctx, lengths=lengths)
    loss2.backward()
    assert torch.equal(loss2.detach(), loss.detach())
    assert bool((ctx.grad[1, :, cut:] == 0).all()), "padded columns of the context received a gradient"
    assert float(ctx.grad[1, :, :cut - 1].abs().max()) > 0 and float(ctx.grad[0, :, cut:].abs().max()) > 0


def test_bf16_context_forward_against_fp32():
    import bf16_ctx_emulation as EC
    cfg, sd, dims, T, idx, feats = _case(64)
    x, f = one_hot(idx, 64).to(DEV), feats.to(DEV)
    exact = _model(64).eval()
    half = _model(64).eval()
    half.forward_precision, half.bf16_context = "bf16", True
    with torch.no_grad():
        want = exact(x, local_features=f, output_unnormalized=False).cpu()
        got = half(x, local_features=f, output_unnormalized=False).cpu()
        ctx = ops.upsample_features(exact, f, T).cpu()
        dec = {k: v for k, v in sd.items() if not k.startswith(("local_conv", "video_"))}
        emu = EC.logits(dec, dims, one_hot(idx, 64), ctx)[:, :, :-1]
    e_got, e_emu = rel_err(got, want), rel_err(emu, want)
    print(f"bf16 with local features: logits rel. err HIP {e_got:.2e}, emulation {e_emu:.2e}")
    assert not torch.equal(got, want) and e_got <= 2 * e_emu, (e_got, e_emu)
    half.bf16_context = False
    with pytest.raises(ValueError, match="bf16"):
        half(x, local_features=f)


def test_greedy_generate_equals_ring_generator_and_oracle():
    cfg, sd, dims, T, idx, feats = _case(32, 3.0)
    rf = dims.receptive_fields
    m = _model(32, 3.0)
    f = feats.to(DEV)
    prompt = one_hot(idx[:, :rf], 64).to(DEV)
    m.generate_local_features = f   # (generate() keeps the reference's signature: the frames are a setting)
    out = m.generate(prompt, n_samples=T, temperature=0.0).argmax(1)
    with torch.no_grad():
        ctx = ops.upsample_features(m, f, T)
    _, _, variant = auto_plan(m._dims, B, True, guided=False)
    gen = RingGenerator(**cfg, state_dict=m._decoder_state(), batch=B, n_total=T, device=DEV, variant=variant,
                        temperature=0.0, context=ctx)
    gen.prime(idx[:, :rf].to(DEV))
    gen.advance(T - rf)
    gen.check_errors()
    assert torch.equal(out.to(torch.int32), gen.samples.to(torch.int32))
    dec = {k: v for k, v in sd.items() if not k.startswith("local_conv")}
    ridx, _ = O.generate_ring(dec, dims, idx[:, :rf].numpy(), T, context=_context64(sd, feats, T).float().numpy())
    assert np.array_equal(out.cpu().numpy(), ridx)
    plain, _ = O.generate_ring(dec, dims, idx[:, :rf].numpy(), T)
    assert not np.array_equal(plain, ridx)   # the features steer the samples


def test_a_length_off_a_multiple_of_four_takes_the_same_paths():
    """T = RF + 41 = 49: the up-sampler's rows are padded to 52 columns and its result is a strided view of them --
    what odd native clip lengths produce -- through forward, score and generate."""
    cfg, sd, dims, T, idx, feats = _case(32, 3.0, 41)
    assert T % 4 == 1
    rf = dims.receptive_fields
    m = _model(32, 3.0).eval()
    m.load_state_dict(sd, strict=False)
    x, f = one_hot(idx, 64).to(DEV), feats.to(DEV)
    dec = {k: v for k, v in sd.items() if not k.startswith("local_conv")}
    ctx64 = _context64(sd, feats, T)
    with torch.no_grad():
        ctx = ops.upsample_features(m, f, T)
        assert tuple(ctx.shape) == (B, 32, T) and not ctx.is_contiguous()
        assert rel_err(ctx.cpu(), ctx64) < 1e-5
        got = m(x, local_features=f, output_unnormalized=False)
        assert torch.equal(got, ops.wavenet_forward(m, x, context=ctx.contiguous(), output_unnormalized=False))
        want = O.forward(dec, dims, one_hot(idx, 64), context=ctx64.float(), output_unnormalized=False)
    assert rel_err(got.cpu(), want) < 2e-5
    assert torch.equal(m.score(x, local_features=f).nll, m.score(x, local_features=f.clone()).nll)
    m.generate_local_features = f
    out = m.generate(x[:, :, :rf], n_samples=T, temperature=0.0).argmax(1)
    ridx, _ = O.generate_ring(dec, dims, idx[:, :rf].numpy(), T, context=ctx64.float().numpy())
    assert np.array_equal(out.cpu().numpy(), ridx)
    assert m.generate_local_features is None   # one call used the setting up


def test_guided_labelled_generate_runs_and_equals_a_guided_ring_generator():
    cfg, sd, dims, T, idx, feats = _case(32, 3.0)
    rf = dims.receptive_fields
    torch.manual_seed(3)
    m = _model(32, 3.0, global_classes=3)
    m.generate_guidance = 1.5
    labels = torch.tensor([2, 0])
    f = feats.to(DEV)
    m.generate_local_features = f
    out = m.generate(one_hot(idx[:, :rf], 64).to(DEV), None, labels, n_samples=T, temperature=0.0).argmax(1)
    with torch.no_grad():
        ctx = ops.upsample_features(m, f, T)
        gvec = m.global_embedding.weight[labels.to(DEV)].detach().float().contiguous()
    _, _, variant = auto_plan(m._dims, B, True, guided=True)
    gen = RingGenerator(**cfg, state_dict=m._decoder_state(), batch=B, n_total=T, device=DEV, variant=variant,
                        temperature=0.0, seed=0, context=ctx, global_context=gvec, guidance=[1.5] * B)
    gen.prime(idx[:, :rf].to(DEV))
    gen.advance(T - rf)
    gen.check_errors()
    assert torch.equal(out.to(torch.int32), gen.samples[-B:].to(torch.int32))


def test_score_tells_true_features_from_rolled_ones():
    cfg, sd, dims, T, idx, feats = _case()
    m = _model().eval()
    x, f = one_hot(idx, 64).to(DEV), feats.to(DEV)
    true, rolled = m.score(x, local_features=f), m.score(x, local_features=f.roll(1, 0))
    assert bool(torch.isfinite(true.nll).all()) and not torch.equal(true.nll, rolled.nll)
    assert torch.equal(true.nll, m.score(x, local_features=f).nll)


def test_trainer_smoke_with_mel(tmp_path):
    from movenet_amd import checkpoint
    from movenet_amd.config import ModelConfig, TrainingConfig
    from movenet_amd.pytorch_lightning_trainer import train_model
    from movenet_amd.wavenet import WaveNet
    mc = ModelConfig(layer_size=2, stack_size=2, input_channels=64, residual_channels=32, skip_channels=32)
    cfg = TrainingConfig(model_config=mc, batch_size=2, val_batch_size=2, n_epochs=1, n_steps_per_epoch=2, use_video=False,
                         use_mel=True, mel_bins=M, mel_fft=64, mel_hop=HOP, scheduler=None, model_output_path=tmp_path,
                         log_samples_every=1, generate_temperature=0.0, score_samples=True)
    tr = train_model("synthetic://clips=4,frames=200,seed=2", cfg)
    assert len(tr.history) == 2 and all(np.isfinite(h["train_loss"]) for h in tr.history)
    path = next((tmp_path / "checkpoints").glob("*.ckpt"))
    ck = torch.load(path, weights_only=True)
    assert ck["local_conditioning"] == {"local_channels": M, "local_hop": HOP, "mel_fft": 64, "mel_fmin": 0.0,
                                        "mel_fmax": 8000.0, "audio_rate": 16000}
    assert "model.local_conv.weight" in ck["state_dict"]
    fresh = WaveNet(2, 2, 64, 32, 32)
    checkpoint.load_into(fresh, path)
    assert (fresh.local_channels, fresh.local_hop) == (M, HOP)
    assert torch.equal(fresh.local_conv.weight, ck["state_dict"]["model.local_conv.weight"])
    rows = [json.loads(line) for line in open(tmp_path / "samples" / "index.jsonl")]
    assert rows and all(r["conditioning"] == "mel" for r in rows if "gen_audio" in r)
    assert any("gen_audio" in r and np.isfinite(r["bits_per_sample"]) for r in rows)
