"""GPU: the opt-in bf16 training mode (WaveNet.forward_precision = "bf16", Trainer(precision="bf16")).

The layers' products run on bf16 operands with fp32 accumulation (mvn_forward_bf16 / mvn_backward_bf16); the
yardstick is tests/bf16_emulation.py, the same rounding points on the fp32 oracle.  Accumulation order alone moves
values across bf16 rounding boundaries, so the criteria are norm- and cosine-level, calibrated against the
emulation on the same input: logits error <= 2 x the emulation's, every parameter gradient's cosine with the fp32
oracle >= min(0.99, the emulation's worst - 0.005), gradient norms within 3 % (or 1.5 x the emulation's own
deviation where that is larger)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bf16_emulation as E
from helpers import one_hot, rel_err, synthetic_indices, weights_of
from movenet_amd import _native as N
from movenet_amd.utils.weights import make_state_dict
from oracle import wavenet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _model(cfg, sd, precision="bf16"):
    from movenet_amd.wavenet import WaveNet
    m = WaveNet(**cfg)
    m.load_state_dict(sd, strict=True)
    m.forward_precision = precision
    return m.to(DEV)


def _cos(a, b) -> float:
    a, b = a.double().flatten(), b.double().flatten()
    return (a @ b / (a.norm() * b.norm()).clamp_min(1e-300)).item()


def _norm_dev(a, ref) -> float:
    return abs(a.double().norm().item() - ref.double().norm().item()) / ref.double().norm().item()


def _check_grads(got, oracle, emu, what):
    """Every oracle gradient: cosine >= min(0.99, emulation's worst - 0.005); norm within 3 % of the oracle's, or
    within 1.5 x the emulation's worst norm deviation where the spec itself moves norms further (measured: up to
    7.4 % on the T = RF + 1 shape, 5.6 % on the Q = 128 one -- the G4 shape stays under 3 %)."""
    assert sorted(got) == sorted(oracle), what
    emu_min = min(_cos(emu[k], oracle[k]) for k in oracle)
    floor = min(0.99, emu_min - 0.005)
    worst = min((_cos(got[k].cpu(), oracle[k]), k) for k in oracle)
    assert worst[0] >= floor, (what, worst, emu_min)
    tol = max(0.03, 1.5 * max(_norm_dev(emu[k], oracle[k]) for k in oracle))
    for k in oracle:
        assert _norm_dev(got[k].cpu(), oracle[k]) <= tol, (what, k, _norm_dev(got[k].cpu(), oracle[k]), tol)
    return worst[0], emu_min


def _loss_step(cfg, sd, x, dims):
    """(loss, grads) of the trainer's step: bf16 HIP, fp32 oracle, the emulation."""
    m = _model(cfg, sd)
    from movenet_amd.ops import wavenet_forward_loss
    loss, _acc, _probs = wavenet_forward_loss(m, x)
    loss.backward()
    assert N.lib().mvn_last_backward_form() == N.BWD_FORM_BF16
    got = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    xc = x.cpu()
    rf = dims.receptive_fields
    target = xc[:, :, rf:].argmax(1)

    def ce(fwd):
        return lambda p: F.cross_entropy(F.softmax(fwd(p)[:, :, :-1], dim=1), target)

    l_ref, g_ref = E.grads_of(ce(lambda p: O.logits_full(p, dims, xc)), sd)
    _l_emu, g_emu = E.grads_of(ce(lambda p: E.logits(p, dims, xc)), sd)
    return loss.item(), got, l_ref.item(), g_ref, g_emu


def _logits_step(cfg, sd, x, dims, seed=11):
    """forward(output_unnormalized=False) with a random upstream gradient: (logits, grads) bf16 / oracle / emulation."""
    m = _model(cfg, sd)
    out = m(x, output_unnormalized=False)
    gen = torch.Generator().manual_seed(seed)
    up = torch.randn(out.shape, generator=gen)
    (out * up.to(DEV)).sum().backward()
    assert N.lib().mvn_last_backward_form() == N.BWD_FORM_BF16
    got = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    xc = x.cpu()
    ref_logits = O.logits_full(sd, dims, xc)[:, :, :-1]
    emu_logits = E.logits(sd, dims, xc)[:, :, :-1].detach()
    _, g_ref = E.grads_of(lambda p: (O.logits_full(p, dims, xc)[:, :, :-1] * up).sum(), sd)
    _, g_emu = E.grads_of(lambda p: (E.logits(p, dims, xc)[:, :, :-1] * up).sum(), sd)
    return out.detach().cpu(), ref_logits, emu_logits, got, g_ref, g_emu


def _fixture_case(golden):
    fx = golden("g4_l30_train.npz")
    cfg, dims, sd = weights_of(fx)
    Q = cfg["input_channels"]
    x = one_hot(synthetic_indices(int(fx["B"]), int(fx["T"]), Q, int(fx["idx_seed"])), Q).to(DEV)
    return fx, cfg, dims, sd, x


def _case(layer_size, stack_size, Q, B, T, seed=7):
    cfg = dict(layer_size=layer_size, stack_size=stack_size, input_channels=Q, residual_channels=64, skip_channels=64)
    sd = make_state_dict(**cfg, seed=seed)
    x = one_hot(synthetic_indices(B, T, Q, seed + 1), Q).to(DEV)
    return cfg, O.Dims(**cfg), sd, x


# ---- 1. forward ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["g4_l30", "reference_q128"])
def test_bf16_forward_logits(golden, shape):
    if shape == "g4_l30":
        _, cfg, dims, sd, x = _fixture_case(golden)
    else:  # the reference's experiment shape: Q = 128, C = K = 64, 10 x 3
        cfg, dims, sd, x = _case(10, 3, 128, 2, 3200)
    with torch.no_grad():
        got = _model(cfg, sd)(x, output_unnormalized=False).cpu()
        exact = _model(cfg, sd, "fp32")(x, output_unnormalized=False).cpu()
    ref = O.logits_full(sd, dims, x.cpu())[:, :, :-1]
    with torch.no_grad():
        emu = E.logits(sd, dims, x.cpu())[:, :, :-1]
    e_got, e_emu = rel_err(got, ref), rel_err(emu, ref)
    print(f"{shape}: logits rel. err bf16 HIP {e_got:.2e}, emulation {e_emu:.2e}, fp32 HIP {rel_err(exact, ref):.2e}")
    assert e_got <= 2 * e_emu, (e_got, e_emu)
    assert not torch.equal(got, exact)  # the bf16 kernels ran


# ---- 2. backward --------------------------------------------------------------------------------------------------
def test_bf16_backward_trainer_loss_g4(golden):
    fx, cfg, dims, sd, x = _fixture_case(golden)
    loss, got, l_ref, g_ref, g_emu = _loss_step(cfg, sd, x, dims)
    worst, emu_min = _check_grads(got, g_ref, g_emu, "g4 loss")
    print(f"g4 loss: bf16 {loss:.7f} oracle {l_ref:.7f} G4 {float(fx['loss']):.7f}; worst cosine {worst:.5f} "
          f"(emulation {emu_min:.5f})")
    assert abs(loss - float(fx["loss"])) < 1e-4


@pytest.mark.parametrize("shape", ["g4_l30", "reference_q128"])
def test_bf16_backward_logits(golden, shape):
    if shape == "g4_l30":
        _, cfg, dims, sd, x = _fixture_case(golden)
    else:
        cfg, dims, sd, x = _case(10, 3, 128, 2, 3200)
    out, ref, emu, got, g_ref, g_emu = _logits_step(cfg, sd, x, dims)
    assert rel_err(out, ref) <= 2 * rel_err(emu, ref)
    worst, emu_min = _check_grads(got, g_ref, g_emu, shape)
    print(f"{shape} logits backward: worst cosine {worst:.5f} (emulation {emu_min:.5f})")


# ---- 3. ragged shapes (guard bands on: conftest.py) ----------------------------------------------------------------
RAGGED = {
    "b1": (10, 3, 256, 1, 3200),
    "b3_t_not_64": (10, 3, 256, 3, 3170),
    "t_rf_plus_1": (10, 3, 256, 2, 3073),        # RF = 3072: one output column
    "stack_2x2": (2, 2, 256, 2, 300),
    "dilation_past_span": (10, 1, 64, 2, 1025),  # the last layer's d = 512 > its 2 valid columns
}


@pytest.mark.parametrize("name", sorted(RAGGED))
def test_bf16_ragged_shapes(name):
    cfg, dims, sd, x = _case(*RAGGED[name])
    assert x.shape[2] >= dims.receptive_fields
    loss, got, l_ref, g_ref, g_emu = _loss_step(cfg, sd, x, dims)
    assert abs(loss - l_ref) < 1e-4, (loss, l_ref)
    _check_grads(got, g_ref, g_emu, name + " loss")
    out, ref, emu, got, g_ref, g_emu = _logits_step(cfg, sd, x, dims)
    assert rel_err(out, ref) <= 2 * rel_err(emu, ref)
    _check_grads(got, g_ref, g_emu, name + " logits")


# ---- 4. refusals --------------------------------------------------------------------------------------------------
def test_bf16_refusals():
    from movenet_amd.ops import wavenet_forward_loss
    from movenet_amd.pytorch_lightning_trainer import Trainer
    cfg = dict(layer_size=2, stack_size=2, input_channels=64, residual_channels=16, skip_channels=16)
    sd = make_state_dict(**cfg, seed=3)
    x = one_hot(synthetic_indices(1, 64, 64, 4), 64).to(DEV)
    m = _model(cfg, sd)
    with pytest.raises(ValueError, match="residual_channels = skip_channels = 64"):
        m(x)
    with pytest.raises(ValueError, match="residual_channels = skip_channels = 64"):
        wavenet_forward_loss(m, x)
    cfg64 = dict(cfg, residual_channels=64, skip_channels=64)
    m64 = _model(cfg64, make_state_dict(**cfg64, seed=3))
    video = torch.zeros(1, 1, 64, 64, 3, device=DEV)
    with pytest.raises(ValueError, match="no video context"):
        m64(x, video)
    ctx = torch.zeros(1, 64, 64, device=DEV)
    with pytest.raises(ValueError, match="no video context"):
        wavenet_forward_loss(m64, x, ctx)
    with pytest.raises(NotImplementedError):
        Trainer(max_epochs=1, precision=16)
    m64.forward_precision = "fp16"  # fp16 stays inference-only
    with pytest.raises(RuntimeError, match="inference-only"):
        m64(x)


# ---- 5. the trainer -----------------------------------------------------------------------------------------------
def test_trainer_bf16_fit(tmp_path):
    from movenet_amd.config import ModelConfig, TrainingConfig
    from movenet_amd.pytorch_lightning_trainer import Dance2Music, Trainer
    mc = ModelConfig(layer_size=4, stack_size=2, input_channels=64, residual_channels=64, skip_channels=64)
    spec = "synthetic://clips=6,frames=600,seed=5"
    sd0 = make_state_dict(4, 2, 64, 64, 64, seed=5)
    runs = {}
    for prec in (32, "bf16"):
        cfg = TrainingConfig(model_config=mc, batch_size=2, val_batch_size=2, n_epochs=2, use_video=False,
                             optimizer="AdamW", learning_rate=3e-3, weight_decay=0.01,
                             model_output_path=tmp_path / str(prec), gradient_clipping=0.0)
        m = Dance2Music(spec, cfg)
        m.model.load_state_dict(sd0)
        tr = Trainer(max_epochs=cfg.n_epochs, default_root_dir=tmp_path / str(prec), precision=prec)
        tr.fit(m)
        runs[prec] = (m, tr, N.lib().mvn_last_backward_form())
    m, tr, form = runs["bf16"]
    assert m.precision == "bf16" and m.model.forward_precision == "bf16" and form == N.BWD_FORM_BF16
    assert runs[32][2] == N.BWD_FORM_ONE and runs[32][0].model.forward_precision == "fp32"
    losses = [h["train_loss"] for h in tr.history]
    assert len(losses) == 6 and np.isfinite(losses).all()
    moved = max((p.detach().cpu() - sd0[k]).abs().max().item() for k, p in m.model.named_parameters())
    assert moved > 1e-4
    # reported, not asserted: AdamW steps of noise-level gradients are not comparable element-wise
    print("fp32 losses:", [round(h["train_loss"], 6) for h in runs[32][1].history])
    print("bf16 losses:", [round(v, 6) for v in losses])
