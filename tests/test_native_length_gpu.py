"""GPU: training and scoring on sequences of their own length, at the model level (WaveNet.forward / score with
``lengths``).

Model 2 x 2 layers, Q = 64, C = K = 64 (the fused path), B = 3, T = RF + 130 -- 130 loss columns, two 64-column tiles
and one of two -- with lengths [T, RF + 65, RF - 1]: a full row, one cut inside the second tile, one shorter than the
receptive field.  The masked loss is held to the EXISTING unmasked call on each clip truncated to its length,
sum_b valid_b loss_b / sum_b valid_b, under the bound test_loss_rule_model_gpu.py holds the same loss to against
float64 (2e-6); parameter gradients under that file's gradient bound (rel_err < 2e-5)."""
import math

import pytest
import torch

from helpers import one_hot, rel_err, synthetic_indices
from movenet_amd.utils.weights import make_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG = dict(layer_size=2, stack_size=2, input_channels=64, residual_channels=64, skip_channels=64)
Q, B, COLS = 64, 3, 130
LOSS_TOL, GRAD_TOL = 2e-6, 2e-5      # test_loss_rule_model_gpu.py: the loss against float64; gradients, rel_err


def _model(rule, precision=None):
    from movenet_amd.wavenet import WaveNet
    m = WaveNet(**CFG)
    m.load_state_dict(make_state_dict(**CFG, seed=11), strict=True)
    m.loss_rule = rule
    if precision is not None:
        m.forward_precision = precision
    return m.to(DEV).train()


def _case(m, seed=3):
    rf = m.receptive_fields
    T = rf + COLS
    lengths = [T, rf + 65, rf - 1]
    valid = [COLS, 65, 0]
    return one_hot(synthetic_indices(B, T, Q, seed), Q).to(DEV), lengths, valid


def _grads(m):
    got = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    return got


def _per_clip(m, x, lengths, valid):
    """sum_b valid_b loss_b / sum_b valid_b (and the accuracy likewise) from the unmasked call on each truncated clip"""
    loss = acc = 0.0
    for b, (n, v) in enumerate(zip(lengths, valid)):
        if v == 0:
            continue
        with torch.no_grad():
            lb, ab, _ = m(x[b:b + 1, :, :n].contiguous(), return_loss=True)
        loss += v * lb.double().item()
        acc += v * ab.double().item()
    return loss / sum(valid), acc / sum(valid)


@pytest.mark.parametrize("rule", ["reference", "model"])
def test_masked_loss_is_the_weighted_mean_of_the_truncated_clips(rule):
    m = _model(rule)
    x, lengths, valid = _case(m)
    want_loss, want_acc = _per_clip(m, x, lengths, valid)
    for given in (lengths, torch.tensor(lengths), torch.tensor(lengths, device=DEV)):
        loss, acc, probs = m(x, return_loss=True, lengths=given)
        print(f"{rule}: masked loss {loss.item():.7f} per-clip {want_loss:.7f}; accuracy {acc.item():.6f} {want_acc:.6f}")
        assert abs(loss.item() - want_loss) < LOSS_TOL
        assert abs(acc.item() - want_acc) < 1e-6
    with torch.no_grad():
        assert torch.equal(probs, m(x))                     # every column's probabilities, padding included
    # no lengths: today's node, and full lengths give its loss
    l0, a0, _ = m(x, return_loss=True)
    l1, a1, _ = m(x, return_loss=True, lengths=[x.shape[2]] * B)
    assert abs(l1.item() - l0.item()) < LOSS_TOL and abs(a1.item() - a0.item()) < 1e-6


@pytest.mark.parametrize("rule", ["reference", "model"])
def test_padding_and_short_rows_do_not_reach_the_gradients(rule):
    m = _model(rule)
    x, lengths, valid = _case(m)
    loss, _, _ = m(x, return_loss=True, lengths=lengths)
    loss.backward()
    want = _grads(m)
    assert want and all(bool(torch.isfinite(g).all()) for g in want.values())
    assert max(float(g.abs().max()) for g in want.values()) > 0
    # other classes in the padding of row 1 and in ALL of row 2 (shorter than the receptive field: nothing counts)
    other = one_hot(synthetic_indices(B, x.shape[2], Q, 99), Q).to(DEV)
    x2 = x.clone()
    x2[1, :, lengths[1]:] = other[1, :, lengths[1]:]
    x2[2] = other[2]
    assert not torch.equal(x2, x)
    loss2, _, _ = m(x2, return_loss=True, lengths=lengths)
    assert abs(loss2.item() - loss.item()) < LOSS_TOL
    loss2.backward()
    got = _grads(m)
    assert sorted(got) == sorted(want)
    worst = max((rel_err(got[k].cpu(), want[k].cpu()), k) for k in want)
    print(f"{rule}: worst gradient rel_err with the padding replaced {worst[0]:.2e} ({worst[1]})")
    assert worst[0] < GRAD_TOL, worst
    # ... and the gradients are those of the truncated clips, weighted
    acc = None
    for b, (n, v) in enumerate(zip(lengths, valid)):
        if v == 0:
            continue
        lb, _, _ = m(x[b:b + 1, :, :n].contiguous(), return_loss=True)
        (lb * (v / sum(valid))).backward()
    per_clip = _grads(m)
    worst = max((rel_err(want[k].cpu(), per_clip[k].cpu()), k) for k in per_clip)
    print(f"{rule}: worst gradient rel_err against the per-clip runs {worst[0]:.2e} ({worst[1]})")
    assert worst[0] < GRAD_TOL, worst


@pytest.mark.parametrize("rule", ["reference", "model"])
def test_all_empty_batch(rule):
    m = _model(rule)
    x, _, _ = _case(m)
    loss, acc, _ = m(x, return_loss=True, lengths=[0, 0, 0])
    assert loss.item() == 0.0 and acc.item() == 0.0
    loss.backward()
    got = _grads(m)
    assert got and all(bool(torch.isfinite(g).all()) and not bool(g.any()) for g in got.values())


def test_score_with_lengths_is_the_model_rule_loss():
    m = _model("model")
    x, lengths, valid = _case(m)
    with torch.no_grad():
        loss, acc, _ = m(x, return_loss=True, lengths=lengths)
    res = m.score(x, lengths=lengths, entropy=True, rank=True)
    assert res.positions.tolist() == valid and res.positions.dtype == torch.int32
    assert abs(res.nll.double().sum().item() / sum(valid) - loss.item()) < LOSS_TOL
    for b, v in enumerate(valid):
        assert bool((res.logp[b, v:] == 0).all()) and bool((res.entropy[b, v:] == 0).all())
        assert bool((res.rank[b, v:] == -1).all()) and bool((res.rank[b, :v] >= 0).all())
    per = torch.tensor([max(v, 1) for v in valid], device=DEV, dtype=torch.float32)
    assert torch.equal(res.bits_per_sample, res.nll / (per * math.log(2.0)))
    assert abs((res.accuracy * per).sum().item() / sum(valid) - acc.item()) < 1e-6
    assert res.nll[2].item() == 0.0 and res.accuracy[2].item() == 0.0
    full = m.score(x)                                        # no lengths: every position, as before
    assert full.positions.tolist() == [COLS] * B and torch.equal(full.logp[0], res.logp[0])


def test_masked_loss_bf16():
    """bf16, audio only: against its own per-clip bf16 runs"""
    m = _model("model", precision="bf16")
    x, lengths, valid = _case(m)
    want_loss, want_acc = _per_clip(m, x, lengths, valid)
    loss, acc, _ = m(x, return_loss=True, lengths=lengths)
    print(f"bf16: masked loss {loss.item():.7f} per-clip {want_loss:.7f}; accuracy {acc.item():.6f} {want_acc:.6f}")
    assert math.isfinite(loss.item()) and abs(loss.item() - want_loss) < LOSS_TOL
    assert abs(acc.item() - want_acc) < 1e-6


def test_masked_loss_with_labels():
    """the label path shares the loss node: lengths with global_features, against the per-clip labelled runs"""
    from movenet_amd.wavenet import WaveNet
    torch.manual_seed(5)
    m = WaveNet(**CFG, global_classes=3)
    sd = m.state_dict()
    sd.update(make_state_dict(**CFG, seed=11))
    m.load_state_dict(sd, strict=True)
    m.loss_rule = "model"
    m = m.to(DEV).train()
    x, lengths, valid = _case(m)
    labels = torch.tensor([2, 0, 1])
    loss, acc, _ = m(x, global_features=labels, return_loss=True, lengths=lengths)
    want_loss = want_acc = 0.0
    for b, (n, v) in enumerate(zip(lengths, valid)):
        if v:
            with torch.no_grad():
                lb, ab, _ = m(x[b:b + 1, :, :n].contiguous(), global_features=labels[b:b + 1], return_loss=True)
            want_loss, want_acc = want_loss + v * lb.item() / sum(valid), want_acc + v * ab.item() / sum(valid)
    assert abs(loss.item() - want_loss) < LOSS_TOL and abs(acc.item() - want_acc) < 1e-6
    loss.backward()
    got = _grads(m)
    assert "global_embedding.weight" in got and all(bool(torch.isfinite(g).all()) for g in got.values())
    assert not bool(got["global_embedding.weight"][1].any())        # row 2's label: nothing of that row counts


def test_trainer_fit_on_a_folder_by_rate(tmp_path, monkeypatch):
    """two optimizer steps of Trainer.fit on three files of different rates and durations with clip_length native: the
    lengths reach the steps, which log the share of loss columns that count"""
    import os
    import movenet_amd.wavenet as W
    import wav_material as M
    from movenet_amd.config import ModelConfig, TrainingConfig, arg_parser, config_from_args
    from movenet_amd.pytorch_lightning_trainer import Dance2Music, Trainer
    clips = [("a_8k", 8000, 1600, 1), ("b_16k", 16000, 4000, 2), ("c_44k", 44100, 30000, 2)]   # 3200, 4000, 8000 (head)
    for split in ("train", "valid"):
        d = tmp_path / "wavs" / split / "a"
        os.makedirs(d)
        for seed, (name, rate, frames, ch) in enumerate(clips):
            M.write_wav(str(d / (name + ".wav")), M.quantise(M.signal("sines", rate, frames, ch, seed), 2), rate)
    args = arg_parser().parse_args(["--dataset", str(tmp_path / "wavs"), "--use_video", "0", "--clip_length", "native"])
    assert config_from_args(args).clip_length == "native"
    cfg = TrainingConfig(model_config=ModelConfig(layer_size=2, stack_size=2, input_channels=64, residual_channels=32,
                                                  skip_channels=32),
                         batch_size=3, val_batch_size=3, n_epochs=2, use_video=False, optimizer="AdamW",
                         learning_rate=1e-3, weight_decay=0.0, scheduler=None, model_output_path=tmp_path,
                         loss_rule="model", clip_length="native", audio_rate=16000)
    m = Dance2Music(str(tmp_path / "wavs"), cfg)
    m2 = Dance2Music(str(tmp_path / "wavs"), TrainingConfig.from_json(cfg.to_json().replace('"native"', '"resample"')))
    # rows of 8000 samples instead of 160 000 (the models are built: the width enters the loaders only from here on)
    monkeypatch.setattr(W, "MAX_AUDIO_FRAMES", 8000)
    tr = Trainer(max_epochs=2, default_root_dir=None, gradient_clip_val=0.0, limit_val_batches=1)
    tr.fit(m)
    assert len(tr.history) == 2
    rf = m.model.receptive_fields
    want = ((3200 - rf) + (4000 - rf) + (8000 - rf)) / (3 * (8000 - rf))
    for h in tr.history:
        assert 0.0 < h["train_valid_frac"] < 1.0 and abs(h["train_valid_frac"] - want) < 1e-9
        assert math.isfinite(h["train_loss"])
    assert 0.0 < m.logged["val_valid_frac"] < 1.0
    # the same folder under the default: no lengths, nothing logged about them
    tr2 = Trainer(max_epochs=1, default_root_dir=None, gradient_clip_val=0.0, limit_val_batches=1)
    tr2.fit(m2)
    assert "train_valid_frac" not in tr2.history[0]
