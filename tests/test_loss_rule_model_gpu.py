"""GPU: the "model" loss rule (WaveNet.loss_rule = "model", --loss_rule model) from the public interface down.

* End to end on the trainer fixtures G4 (generic kernels; fused C = K = 64 path): the probabilities and the accuracy
  are the reference rule's, the loss is float64 cross_entropy of the forward's own logits within 2e-6 (the bound
  test_trainer_fused_gpu.py holds the reference rule's loss to), and the parameter gradients equal those of the
  float64 gradient 2 (softmax - onehot) / (B S), cast to fp32 and fed through the unfused node: both sides run the
  same mvn_backward, so they differ by the fp32 rounding of dlogit only -- rel_err < 2e-5, the project's
  fp32-against-float64 tolerance.  (For scale, the test prints the same comparison for torch's own fp32
  F.cross_entropy through the unfused node.)  Explicit targets, dense (soft) input, a context tensor, bf16.
* Learning, in the setting of test_audio_frontend_gpu.py's learning test (four two-sine clips, 4 x 2 layers, C = K = 32,
  Q = 64, AdamW 3e-3, 400 steps of 2 clips x 4000 frames).  The CPU oracle (oracle/wavenet_oracle.py unchanged,
  F.cross_entropy on its logits, torch's AdamW, the loader's clip order and crops restated on the host) ends at NLL
  0.1729 nats, accuracy 0.935 (mean of the last 10 % of the steps; 0.1720 with another thread count), from 4.186 at
  the first step.  The reference rule cannot leave [ln Q - 1, ln Q] = [3.159, 4.159] by construction.  Bounds: first
  step within 5 % of ln Q; final NLL <= 1.25 x the oracle's and below ln Q - 1; accuracy > 10 / Q; the synthetic://
  noise control within 5 % of ln Q; train_bits_per_sample logged and equal to train_loss / ln 2.  Measured on an
  MI355X: first step 4.187, final NLL 0.1714, accuracy 0.937 in 2.9 s; noise 4.159 / 0.016 in 1.5 s; worst gradient
  rel_err 7.2e-7 (G4 small) / 5.6e-7 (G4 30 layers), torch's own fp32 cross_entropy 5.6e-7 / 5.1e-7."""
import math
import os
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_rule_reference as R
import wav_material as M
from helpers import one_hot, rel_err, synthetic_indices, weights_of
from movenet_amd import _native as N
from movenet_amd.utils.weights import make_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _model(cfg, sd, rule="model"):
    from movenet_amd.wavenet import WaveNet
    m = WaveNet(**cfg)
    m.load_state_dict(sd, strict=True)
    m.loss_rule = rule
    return m.to(DEV)


def _grads(m):
    got = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    return got


def _ce64(logits, target):
    return F.cross_entropy(logits.detach().double(), target).item()


@pytest.mark.parametrize("name", ["g4_small_train.npz", "g4_l30_train.npz"])
def test_model_rule_end_to_end_on_g4(golden, name):
    from movenet_amd.ops import wavenet_forward, wavenet_forward_loss
    fx = golden(name)
    cfg, dims, sd = weights_of(fx)
    Q, B, T = cfg["input_channels"], int(fx["B"]), int(fx["T"])
    x = one_hot(synthetic_indices(B, T, Q, int(fx["idx_seed"])), Q).to(DEV)
    m = _model(cfg, sd, "reference").train()
    rf = m.receptive_fields
    # the default rule is untouched
    loss_r, acc_r, _ = m(x, return_loss=True)
    assert abs(loss_r.item() - float(fx["loss"])) < 2e-6
    m.loss_rule = "model"
    with torch.no_grad():
        out = m(x)
    target = x[:, :, rf:].argmax(1)
    loss, acc, probs = m(x, return_loss=True)
    assert torch.equal(probs, out) and acc.item() == acc_r.item()
    logits = m(x, output_unnormalized=False)  # (the reference's inverted flag: the raw logits)
    S = logits.shape[2]
    ce = _ce64(logits, target)
    print(f"{name}: loss {loss.item():.7f} float64 CE of the logits {ce:.7f} (reference rule {loss_r.item():.7f})")
    assert abs(loss.item() - ce) < 2e-6
    (2.0 * loss).backward()                    # the upstream gradient is honoured
    got = _grads(m)
    L = cfg["layer_size"] * cfg["stack_size"]
    assert sorted(got) == [str(n) for n in fx["grad_names"]]   # the reference rule's parameter set
    assert not any(k.startswith(f"residual_conv_stack.conv_layers.{L - 1}.conv_residual.") for k in got)
    # the float64 gradient, rounded to fp32 once, through the unfused node's mvn_backward
    g64 = R.model_dlogit(R.model_probs(logits.detach()), target, 2.0 / (B * S))
    logits.backward(g64.float())
    want = _grads(m)
    # for scale: torch's own fp32 cross_entropy through the same node
    logits2 = m(x, output_unnormalized=False)
    (2.0 * F.cross_entropy(logits2, target)).backward()
    torch_fp32 = _grads(m)
    assert sorted(want) == sorted(got) == sorted(torch_fp32)
    worst = max((rel_err(got[k].cpu(), want[k].cpu()), k) for k in want)
    worst_t = max((rel_err(torch_fp32[k].cpu(), want[k].cpu()), k) for k in want)
    print(f"{name}: worst gradient rel_err {worst[0]:.2e} ({worst[1]}); torch fp32 cross_entropy {worst_t[0]:.2e} "
          f"({worst_t[1]})")
    for k in want:
        assert rel_err(got[k].cpu(), want[k].cpu()) < 2e-5, k
    # an explicit target
    tgx = torch.randint(0, Q, (B, S), generator=torch.Generator().manual_seed(5)).to(DEV)
    l2, a2, p2 = wavenet_forward_loss(m, x, target=tgx)
    assert torch.equal(p2, out) and abs(l2.item() - _ce64(logits, tgx)) < 2e-6
    assert a2.item() == (out.argmax(1) == tgx).float().mean().item()
    # a non-one-hot input takes the dense causal conv
    soft = torch.softmax(torch.randn(1, Q, T, device=DEV), 1)
    tg = soft[:, :, rf:].argmax(1)
    l3, a3, p3 = wavenet_forward_loss(m, soft)
    with torch.no_grad():
        ref, lg = m(soft), m(soft, output_unnormalized=False)
    assert torch.equal(p3, ref) and abs(l3.item() - _ce64(lg, tg)) < 2e-6
    assert a3.item() == (ref.argmax(1) == tg).float().mean().item()
    l3.backward()
    assert sorted(_grads(m)) == sorted(want)
    # conditioned: a context tensor on the absolute time axis
    ctx = 0.3 * torch.randn(B, cfg["residual_channels"], T, device=DEV)
    l4, a4, p4 = wavenet_forward_loss(m, x, ctx)
    with torch.no_grad():
        lg4, ref4 = wavenet_forward(m, x, ctx, output_unnormalized=False), wavenet_forward(m, x, ctx)
    assert abs(l4.item() - _ce64(lg4, target)) < 2e-6 and torch.equal(p4, ref4) and not torch.equal(ref4, out)
    l4.backward()
    assert any(".context_conv_" in k for k in _grads(m))
    # ... and the rule can be named per call
    l5, _, _ = wavenet_forward_loss(m, x, loss_rule="reference")
    assert l5.item() == loss_r.item()


def test_model_rule_bf16():
    """the loss kernels see fp32 logits under bf16 as well: the NLL of that forward's own logits"""
    cfg = dict(layer_size=2, stack_size=2, input_channels=256, residual_channels=64, skip_channels=64)
    sd = make_state_dict(**cfg, seed=7)
    x = one_hot(synthetic_indices(2, 300, 256, 8), 256).to(DEV)
    m = _model(cfg, sd)
    m.forward_precision = "bf16"
    target = x[:, :, m.receptive_fields:].argmax(1)
    loss, acc, probs = m(x, return_loss=True)
    with torch.no_grad():
        logits, ref = m(x, output_unnormalized=False), m(x)
    ce = _ce64(logits, target)
    print(f"bf16: loss {loss.item():.7f} float64 CE of its logits {ce:.7f}")
    assert math.isfinite(loss.item()) and abs(loss.item() - ce) < 2e-6
    assert torch.equal(probs, ref) and acc.item() == (ref.argmax(1) == target).float().mean().item()
    loss.backward()
    assert N.lib().mvn_last_backward_form() == N.BWD_FORM_BF16
    got = _grads(m)
    assert got and all(bool(torch.isfinite(g).all()) for g in got.values())


# ---- training has to learn ------------------------------------------------------------------------------------------
ORACLE_FINAL_NLL, ORACLE_FINAL_ACC = 0.1729, 0.935     # CPU oracle, same material / model / optimizer / steps
LEARN_Q, STEPS = 64, 400


def _fit(dataset, tmp_path, epochs):
    from movenet_amd.config import ModelConfig, TrainingConfig
    from movenet_amd.pytorch_lightning_trainer import Dance2Music, Trainer
    mc = ModelConfig(layer_size=4, stack_size=2, input_channels=LEARN_Q, residual_channels=32, skip_channels=32)
    is_dir = os.path.isdir(dataset)
    cfg = TrainingConfig(model_config=mc, batch_size=2, val_batch_size=1, n_epochs=epochs, use_video=False,
                         optimizer="AdamW", learning_rate=3e-3, weight_decay=0.0, scheduler=None,
                         batch_subsample_frac=0.025 if is_dir else None,
                         val_batch_subsample_frac=0.025 if is_dir else None, model_output_path=tmp_path,
                         loss_rule="model")
    m = Dance2Music(dataset, cfg)
    m.model.load_state_dict(make_state_dict(4, 2, LEARN_Q, 32, 32, seed=11))
    tr = Trainer(max_epochs=epochs, default_root_dir=None, gradient_clip_val=0.0, limit_val_batches=1)
    tr.fit(m)
    assert len(tr.history) == STEPS
    for h in tr.history:  # logged beside the loss, the same device scalar over ln 2 (fp32 division)
        assert abs(h["train_bits_per_sample"] - h["train_loss"] / math.log(2.0)) <= 1e-6 * max(1.0, h["train_loss"])
    assert "val_bits_per_sample" in m.logged
    tail = tr.history[-STEPS // 10:]
    return (float(np.mean([h["train_loss"] for h in tail])), float(np.mean([h["train_acc"] for h in tail])),
            tr.history[0]["train_loss"])


def test_training_under_the_model_rule_learns_and_on_noise_does_not(tmp_path):
    """Bounds and the oracle's figures: the module docstring."""
    ln_q = math.log(LEARN_Q)
    root = tmp_path / "tones"
    M.write_learning_tree(root)
    t0 = time.perf_counter()
    nll, acc, nll0 = _fit(str(root), tmp_path, epochs=STEPS // 2)           # 4 clips / batch 2 = 2 steps an epoch
    t1 = time.perf_counter()
    noise_nll, noise_acc, _ = _fit(f"synthetic://clips={STEPS},frames=4000,seed=3", tmp_path, epochs=2)
    t2 = time.perf_counter()
    print(f"waveforms: first step {nll0:.4f}, last 10 % NLL {nll:.4f} acc {acc:.4f} in {t1 - t0:.1f} s "
          f"(oracle {ORACLE_FINAL_NLL} / {ORACLE_FINAL_ACC}); noise: NLL {noise_nll:.4f} acc {noise_acc:.4f} "
          f"in {t2 - t1:.1f} s; ln Q {ln_q:.4f}, ln Q - 1 {ln_q - 1:.4f}")
    assert abs(nll0 - ln_q) < 0.05 * ln_q                       # it starts where noise stays
    assert nll <= 1.25 * ORACLE_FINAL_NLL                       # the existing learning test's margin
    assert nll < ln_q - 1.0                                     # out of the reference rule's reach by construction
    assert acc > 10.0 / LEARN_Q
    assert abs(noise_nll - ln_q) <= 0.05 * ln_q                 # the control: the drop comes from the data
    assert noise_acc < 10.0 / LEARN_Q
