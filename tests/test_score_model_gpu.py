"""GPU: WaveNet.score / WaveNet.classify and the trainer's --score_samples from the public interface down.

``score`` runs the forward's own kernels and hands their logits to mvn_score_columns, so against float64
log_softmax + gather of ``forward(output_unnormalized=False)`` on the same input the only error is that kernel's: the
bounds of test_score_gpu.py (logp max|err| / max|ref| <= 2e-5, nll 1e-5 relative) -- under ``forward_precision =
"bf16"`` too, where the comparison is against the bf16 forward's own logits.  ``classify`` is held to ``score`` called
once per class, and a chunk budget that forces several chunks to the one-chunk result (the test prints whether that
is bit-equal; it asserts the bounds).  Measured on an MI355X: logp at most 0.6 % and nll 1.4 % of their bounds
(fp32, bf16, labelled on both paths, video + label); classify bit-equal to score per class and across chunks of one,
two and nine pairs."""
import json
import math

import numpy as np
import pytest
import torch

from helpers import one_hot, synthetic_indices
from movenet_amd.utils.weights import make_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL, NLL_TOL = 2e-5, 1e-5
BIG = dict(layer_size=2, stack_size=2, input_channels=64, residual_channels=64, skip_channels=64)
SMALL = dict(layer_size=2, stack_size=2, input_channels=16, residual_channels=16, skip_channels=8)


def _model(cfg, G=0, seed=3, **kw):
    from movenet_amd.wavenet import WaveNet
    torch.manual_seed(seed)                               # (the label embedding's default draw)
    m = WaveNet(**cfg, global_classes=G, **kw)
    sd = make_state_dict(**cfg, seed=seed, gain=1.5, **({"context_in_channels": kw["context_in_channels"]}
                                                        if "context_in_channels" in kw else {}))
    m.load_state_dict(sd, strict=False)
    return m.to(DEV).eval()


def _audio(m, B, extra=65, seed=5):
    Q = m.input_channels
    return one_hot(synthetic_indices(B, m.receptive_fields + extra, Q, seed), Q).to(DEV)


def _check(res, logits, x, rf, what):
    """``res`` against float64 log_softmax + gather of ``logits`` (B, Q, S)"""
    target = x[:, :, rf:].argmax(1)
    ls = torch.log_softmax(logits.double(), 1)
    want = ls.gather(1, target[:, None])[:, 0]
    S = want.shape[1]
    assert res.logp.shape == want.shape and res.nll.shape == (x.shape[0],)
    e_lp = ((res.logp.double() - want).abs().max() / want.abs().max()).item()
    e_nll = ((res.nll.double() + want.sum(1)).abs() / want.sum(1).abs()).max().item()
    print(f"{what}: logp err {e_lp:.2e} ({e_lp / TOL:.3f} of its bound), nll err {e_nll:.2e} ({e_nll / NLL_TOL:.3f})")
    assert e_lp <= TOL and e_nll <= NLL_TOL
    assert torch.allclose(res.bits_per_sample.double(), -want.sum(1) / (S * math.log(2.0)), rtol=NLL_TOL, atol=0)
    assert torch.equal(res.accuracy, (logits.argmax(1) == target).float().mean(1))
    return want


@pytest.mark.parametrize("cfg", [BIG, SMALL], ids=["C64_Q64", "C16_K8_Q16"])
def test_score_vs_the_models_own_logits(cfg):
    m = _model(cfg)
    x = _audio(m, 3)
    rf = m.receptive_fields
    with torch.no_grad():
        logits = m(x, output_unnormalized=False)
    res = m.score(x, entropy=True, rank=True)
    want = _check(res, logits, x, rf, "fp32")
    ls = torch.log_softmax(logits.double(), 1)
    ent = -(ls.exp() * ls).sum(1)
    assert ((res.entropy.double() - ent).abs().max() / ent.abs().max()).item() <= TOL
    tl = logits.gather(1, x[:, :, rf:].argmax(1)[:, None])
    assert torch.equal(res.rank.long(), (logits > tl).sum(1))               # (no exact ties in these logits)
    plain = m.score(x)
    assert plain.entropy is None and plain.rank is None and torch.equal(plain.logp, res.logp)
    # temperature: softmax(logits / T)
    hot = m.score(x, temperature=2.0)
    want2 = torch.log_softmax(logits.double() / 2.0, 1).gather(1, x[:, :, rf:].argmax(1)[:, None])[:, 0]
    assert ((hot.logp.double() - want2).abs().max() / want2.abs().max()).item() <= TOL
    # the number loss_rule = "model" reports for the same input
    m.loss_rule = "model"
    with torch.no_grad():
        loss, acc, _ = m(x, return_loss=True)
    mean = (res.nll / (x.shape[2] - rf)).mean().item()
    print(f"mean nll {mean:.7f} loss {loss.item():.7f}")
    assert abs(mean - loss.item()) <= 1e-5 * abs(loss.item())
    assert abs(res.accuracy.mean().item() - acc.item()) < 1e-6
    # not one-hot: there is no target to score
    soft = x.clone()
    soft[0, :, rf + 3] = 1.0 / m.input_channels
    with pytest.raises(ValueError, match="one-hot"):
        m.score(soft)


def test_score_under_bf16_is_held_to_the_bf16_logits():
    m = _model(BIG)
    m.forward_precision = "bf16"
    x = _audio(m, 3)
    with torch.no_grad():
        logits = m(x, output_unnormalized=False)
    _check(m.score(x), logits, x, m.receptive_fields, "bf16")
    m.forward_precision = "fp32"
    with torch.no_grad():
        assert not torch.equal(m(x, output_unnormalized=False), logits)     # (it was the bf16 forward)


def test_score_has_no_side_effects():
    m = _model(BIG)
    x = _audio(m, 2)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    for mode in (True, False):
        m.train(mode)
        res = m.score(x)
        assert m.training is mode
        assert not res.logp.requires_grad and not res.nll.requires_grad
    assert all(p.grad is None for p in m.parameters())
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    with torch.enable_grad():                                               # the caller's grad mode does not matter
        assert not m.score(x).nll.requires_grad


@pytest.mark.parametrize("path", ["auto", "context"])
def test_score_of_a_labelled_model(path):
    m = _model(BIG, G=3)
    m.global_path = path
    m.global_dropout = 1.0                                                  # never applied by score, even in train mode
    x = _audio(m, 3)
    labels = torch.tensor([2, 0, 1])
    with torch.no_grad():
        logits = m(x, None, labels, output_unnormalized=False)              # (eval mode: no dropout)
    m.train()
    res = m.score(x, None, labels)
    assert m.training
    _check(res, logits, x, m.receptive_fields, f"labelled, global_path {path}")
    other = m.score(x, None, torch.tensor([0, 1, 2]))
    assert not torch.equal(other.nll, res.nll)                              # the label is used


def test_score_with_video(monkeypatch):
    """frames in [0, 1], at the shape of test_global_conditioning_gpu.py's label-and-video case"""
    import movenet_amd.wavenet as W
    frames, B, cin = 7, 3, 3
    T = 1000 * frames
    monkeypatch.setattr(W, "MAX_AUDIO_FRAMES", T)
    monkeypatch.setattr(W, "MAX_VIDEO_FRAMES", frames)
    cfg = dict(layer_size=3, stack_size=2, input_channels=256, residual_channels=64, skip_channels=64)
    m = _model(cfg, G=4, seed=29, context_in_channels=cin)
    x = one_hot(synthetic_indices(B, T, 256, 1234), 256).to(DEV)
    video = torch.from_numpy(np.random.default_rng(4321).random((B, frames, 64, 64, cin), dtype=np.float32)).to(DEV)
    labels = torch.tensor([2, 0, 2])
    with torch.no_grad():
        logits = m(x, video, labels, output_unnormalized=False)
    _check(m.score(x, video, labels), logits, x, m.receptive_fields, "video + label")


def test_classify():
    G, B = 3, 3
    m = _model(BIG, G=G)
    x = _audio(m, B)
    loglik, post = m.classify(x)
    assert loglik.shape == (B, G) and post.shape == (B, G)
    per_class = torch.stack([-m.score(x, None, torch.full((B,), c)).nll for c in range(G)], 1)
    e = ((loglik.double() - per_class.double()).abs() / per_class.double().abs()).max().item()
    print(f"classify vs score per class: {e:.2e} ({e / NLL_TOL:.3f} of its bound), bit-equal: "
          f"{torch.equal(loglik, per_class)}")
    assert e <= NLL_TOL
    assert torch.allclose(post.double().sum(1), torch.ones(B, dtype=torch.float64, device=DEV), atol=1e-6)
    assert torch.allclose(post.double(), torch.softmax(loglik.double(), 1), atol=1e-6)
    assert len(set(loglik[0].tolist())) == G                                # the classes are told apart
    # a prior shifts the posterior as Bayes' rule says: posterior' ~ posterior x prior
    prior = torch.tensor([0.7, 0.2, 0.1])
    _, shifted = m.classify(x, log_prior=prior.log())
    want = post.double() * prior.double().to(DEV)
    assert torch.allclose(shifted.double(), want / want.sum(1, keepdim=True), atol=1e-6)
    rows = torch.log(torch.tensor([[0.5, 0.25, 0.25], [0.1, 0.1, 0.8], [1 / 3, 1 / 3, 1 / 3]]))
    _, per_row = m.classify(x, log_prior=rows)
    assert torch.allclose(per_row.double(), torch.softmax(loglik.double() + rows.double().to(DEV), 1), atol=1e-6)
    # several chunks: two (class, sequence) pairs at a time instead of all nine
    per_pair = 4 * m.input_channels * (x.shape[2] - m.receptive_fields)
    chunked, _ = m.classify(x, logits_budget_bytes=2 * per_pair)
    single, _ = m.classify(x, logits_budget_bytes=1)                        # (one pair per chunk)
    for name, other in (("two pairs per chunk", chunked), ("one pair per chunk", single)):
        e = ((other.double() - loglik.double()).abs() / loglik.double().abs()).max().item()
        print(f"{name} vs one chunk: {e:.2e}, bit-equal: {torch.equal(other, loglik)}")
        assert e <= NLL_TOL
    # the forced general path gives the same answer within the forward's own agreement between its two label paths
    m.global_path = "context"
    general, _ = m.classify(x)
    assert ((general.double() - loglik.double()).abs() / loglik.double().abs()).max().item() < 1e-4
    assert not m.training and all(p.grad is None for p in m.parameters())


def _fit(tmp_path, name, score_samples, seen=None):
    from movenet_amd.callbacks import LogSamplesCallback
    from movenet_amd.config import arg_parser, config_from_args
    from movenet_amd.pytorch_lightning_trainer import Dance2Music, Trainer
    out = tmp_path / name
    spec = "synthetic://clips=4,frames=60,seed=2"
    args = arg_parser().parse_args([
        "--dataset", spec, "--use_video", "0", "--use_global", "1", "--log_samples_every", "1",
        "--score_samples", str(score_samples), "--input_channels", "64", "--residual_channels", "16",
        "--skip_channels", "16", "--layer_size", "2", "--stack_size", "2", "--batch_size", "2", "--val_batch_size", "2",
        "--n_epochs", "1", "--num_workers", "0", "--val_num_workers", "0", "--model_output_path", str(out)])
    torch.manual_seed(5)
    module = Dance2Music(spec, config_from_args(args))
    if seen is not None:
        inner = module.score_samples

        def spy(generated, audio, video, labels=None):
            got = inner(generated, audio, video, labels)
            direct = (module.model.score(generated, video, labels).bits_per_sample,
                      module.model.score(audio.to(generated.dtype), video, labels).bits_per_sample)
            seen.append((got, direct))
            return got
        module.score_samples = spy
    trainer = Trainer(max_epochs=1, default_root_dir=str(out), callbacks=[LogSamplesCallback(log_every_n_epochs=1)])
    trainer.fit(module)
    return [json.loads(line) for line in open(out / "samples" / "index.jsonl")]


def test_sample_logger_scores(tmp_path):
    seen = []
    rows = _fit(tmp_path, "on", 1, seen)
    assert rows and seen
    bits = torch.cat([got["bits_per_sample"].cpu() for got, _ in seen]).tolist()
    source = torch.cat([got["source_bits_per_sample"].cpu() for got, _ in seen]).tolist()
    assert [r["bits_per_sample"] for r in rows] == bits and [r["source_bits_per_sample"] for r in rows] == source
    assert all(math.isfinite(v) and v > 0 for v in bits + source)
    for got, (gen_direct, src_direct) in seen:                              # one call for both, equal to a call each
        assert torch.allclose(got["bits_per_sample"], gen_direct, rtol=NLL_TOL, atol=0)
        assert torch.allclose(got["source_bits_per_sample"], src_direct, rtol=NLL_TOL, atol=0)
    off = _fit(tmp_path, "off", 0)
    assert len(off) == len(rows)
    assert not any("bits_per_sample" in r or "source_bits_per_sample" in r for r in off)
    strip = lambda r: {k: v for k, v in r.items() if k not in ("bits_per_sample", "source_bits_per_sample")}
    assert [strip(r) for r in rows] == off                                  # nothing else in a row moves
