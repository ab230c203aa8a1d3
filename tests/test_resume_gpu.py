"""GPU: a run resumed from ``last.ckpt`` is the run that was never interrupted.

The trainer shape of ``test_ema_gpu.py`` (6 noise clips of 600 samples, batch 2: 3 steps per epoch; 4 x 2 layers,
Q = C = K = 64; AdamW with the weights' average, OneCycleLR over 2 epochs, gradients clipped at 1.0), at which two
independent ``fit`` runs give ``torch.equal`` weights -- so the comparisons below are ``torch.equal`` too.

1. Epoch boundary: 1 epoch, then new objects resumed from ``last.ckpt`` for the second, against 2 epochs in one go.
2. Mid-epoch: ``checkpoint_every_n_steps=2``, the run killed inside batch 2 of epoch 0, resumed from ``last.ckpt``.
3. Label dropout: the masks drawn by the interrupted and the resumed run are those of the uninterrupted run.
4. Fine-tuning: ``pretrained_model_path`` loads the weights and nothing else.
5. bf16: test 1's flow under ``precision="bf16"``.
"""
import wave

import numpy as np
import pytest
import torch

from movenet_amd.utils.weights import make_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPEC = "synthetic://clips=6,frames=600,seed=5"
SHAPE = dict(layer_size=4, stack_size=2, input_channels=64, residual_channels=64, skip_channels=64)


class _Killed(Exception):
    pass


class _Batches:
    """Records the ``filepaths`` of every trained batch; ``kill_at``: raises ``_Killed`` in ``on_train_batch_end`` of
    that batch of epoch 0 (after its backward, before its optimizer step)."""

    def __init__(self, kill_at=None):
        self.kill_at, self.seen = kill_at, []

    def on_train_batch_end(self, trainer, module, outputs, batch, batch_idx):
        self.seen.append((trainer.current_epoch, batch_idx, list(batch.filepaths)))
        if self.kill_at is not None and trainer.current_epoch == 0 and batch_idx == self.kill_at:
            assert (trainer.root / "checkpoints" / "last.ckpt").exists()  # (the file of the step before)
            raise _Killed()

    def on_validation_batch_end(self, *a, **k):
        pass


def _objects(root, precision=32, max_epochs=2, callbacks=None, every=0, dataset=SPEC, seed_weights=True, **over):
    from movenet_amd.config import ModelConfig, TrainingConfig
    from movenet_amd.pytorch_lightning_trainer import Dance2Music, Trainer
    kw = dict(model_config=ModelConfig(**SHAPE), batch_size=2, val_batch_size=2, n_epochs=2, use_video=False,
              optimizer="AdamW", learning_rate=3e-3, weight_decay=0.01, model_output_path=root, scheduler="OneCycleLR",
              ema_decay=0.9, gradient_clipping=1.0)
    cfg = TrainingConfig(**{**kw, **over})
    m = Dance2Music(dataset, cfg)
    if seed_weights:
        m.model.load_state_dict(make_state_dict(4, 2, 64, 64, 64, seed=5))
    tr = Trainer(max_epochs=max_epochs, default_root_dir=root, precision=precision, gradient_clip_val=1.0,
                 accumulate_grad_batches=1, callbacks=callbacks, checkpoint_every_n_steps=every)
    return m, tr


def _snapshot(m, tr) -> dict:
    opt = tr.optimizer
    return dict(state={k: v.detach().cpu().clone() for k, v in m.model.state_dict().items()},
                buffers={k: getattr(opt, k).detach().cpu().clone() for k in ("flat", "exp_avg", "exp_avg_sq", "ema")},
                steps=list(opt._steps), ema_updates=opt.ema_updates, lr=opt.param_groups[0]["lr"],
                losses=[h["train_loss"] for h in tr.history], steps_logged=[h["step"] for h in tr.history],
                val=dict(getattr(tr, "val_epoch_means", {})))  # (a run killed inside its first epoch has none)


def _assert_same_run(whole: dict, resumed: dict, first_part: dict) -> None:
    """``resumed`` (the snapshot after the resumed fit) against ``whole``; ``first_part``: the interrupted run's."""
    assert resumed["state"].keys() == whole["state"].keys()
    for k, v in whole["state"].items():
        assert torch.equal(resumed["state"][k], v), k
    for k, v in whole["buffers"].items():
        assert torch.equal(resumed["buffers"][k], v), k
    assert resumed["steps"] == whole["steps"] and resumed["ema_updates"] == whole["ema_updates"] == 6
    assert resumed["lr"] == whole["lr"]
    assert first_part["losses"] + resumed["losses"] == whole["losses"] and len(whole["losses"]) == 6
    assert first_part["steps_logged"] + resumed["steps_logged"] == whole["steps_logged"] == list(range(6))
    assert resumed["val"] == whole["val"]


def _uninterrupted(root, precision=32):
    rec = _Batches()
    m, tr = _objects(root, precision=precision, callbacks=[rec])
    tr.fit(m)
    return dict(_snapshot(m, tr), batches=rec.seen, root=root)


def _epoch_boundary(root, precision=32):
    """(snapshot of the run stopped after epoch 0, snapshot of new objects resumed from its last.ckpt to the end)."""
    m, tr = _objects(root, precision=precision, max_epochs=1)
    tr.fit(m)
    first = _snapshot(m, tr)
    m2, tr2 = _objects(root, precision=precision, seed_weights=False)  # new objects, their own random weights
    tr2.fit(m2, ckpt_path=root / "checkpoints" / "last.ckpt")
    return first, _snapshot(m2, tr2)


@pytest.fixture(scope="module")
def whole(tmp_path_factory):
    """Run A: 2 epochs in one go.  Computed once, read by every test below."""
    return _uninterrupted(tmp_path_factory.mktemp("whole") / "run")


def _load(path):
    return torch.load(path, map_location="cpu", weights_only=True)


def test_checkpoint_files_of_an_uninterrupted_run(whole):
    ck_dir = whole["root"] / "checkpoints"
    assert sorted(p.name for p in ck_dir.iterdir()) == ["epoch=0-step=3.ckpt", "epoch=1-step=6.ckpt", "last.ckpt"]
    last, final = _load(ck_dir / "last.ckpt"), _load(ck_dir / "epoch=1-step=6.ckpt")
    assert set(last) == {"epoch", "global_step", "state_dict", "ema_state_dict", "ema_decay", "ema_updates",
                         "optimizer_states", "lr_schedulers", "hyper_parameters", "resume"} == set(final)
    assert last["epoch"] == 1 and last["global_step"] == 6 and last["ema_updates"] == 6
    assert last["resume"]["epoch"] == 2 and last["resume"]["batches_done"] == 0 and last["resume"]["history_len"] == 6
    assert last["hyper_parameters"] == {**SHAPE, "precision": 32, "bf16_video": False, "loss_rule": "reference",
                                        "optimizer": "AdamW", "scheduler": "OneCycleLR", "accumulation_steps": 1,
                                        "batch_size": 2, "world_size": 1, "dataset": SPEC}
    for k, v in whole["state"].items():
        assert torch.equal(last["state_dict"][f"model.{k}"], v) and torch.equal(final["state_dict"][f"model.{k}"], v)
    flat = last["optimizer_states"][0]["state"]["flat"]
    assert set(flat) == {"steps", "exp_avg", "exp_avg_sq", "ema", "ema_updates"} and flat["ema_updates"] == 6
    assert flat["steps"] == whole["steps"] and all(not t.is_cuda for t in (flat["exp_avg"], flat["exp_avg_sq"], flat["ema"]))
    for k in ("exp_avg", "exp_avg_sq", "ema"):
        assert torch.equal(flat[k], whole["buffers"][k]) and torch.equal(flat[k], final["optimizer_states"][0]["state"]["flat"][k])
    assert last["optimizer_states"][0]["param_groups"][0]["lr"] == whole["lr"]
    assert last["lr_schedulers"][0]["last_epoch"] == 6
    # one host copy per flat buffer: the per-name entries are views of it, and the file holds each buffer once
    n = whole["buffers"]["flat"].numel()
    for key in ("state_dict", "ema_state_dict"):
        stores = {}
        for v in last[key].values():
            stores.setdefault(v.untyped_storage().data_ptr(), v.untyped_storage().nbytes())
        assert max(stores.values()) == 4 * n, key
    assert last["ema_state_dict"]["model.causal_conv.conv.weight"].untyped_storage().data_ptr() == \
        flat["ema"].untyped_storage().data_ptr()
    size = (ck_dir / "last.ckpt").stat().st_size
    assert 4 * 4 * n <= size <= 4 * 4 * n * 1.5  # weights, two moments, average (+ what the optimizer leaves out)
    first = _load(ck_dir / "epoch=0-step=3.ckpt")
    assert first["epoch"] == 0 and first["global_step"] == 3 and first["resume"]["epoch"] == 1


def test_resume_at_an_epoch_boundary(whole, tmp_path):
    first, resumed = _epoch_boundary(tmp_path / "run")
    assert len(first["losses"]) == 3 and len(resumed["losses"]) == 3
    _assert_same_run(whole, resumed, first)
    names = sorted(p.name for p in (tmp_path / "run" / "checkpoints").iterdir())
    assert names == ["epoch=0-step=3.ckpt", "epoch=1-step=6.ckpt", "last.ckpt"]
    a, b = _load(whole["root"] / "checkpoints" / "last.ckpt"), _load(tmp_path / "run" / "checkpoints" / "last.ckpt")
    assert all(torch.equal(a["ema_state_dict"][k], b["ema_state_dict"][k]) for k in a["ema_state_dict"])
    assert torch.equal(a["optimizer_states"][0]["state"]["flat"]["ema"], b["optimizer_states"][0]["state"]["flat"]["ema"])
    assert a["lr_schedulers"] == b["lr_schedulers"] and a["resume"]["epoch"] == b["resume"]["epoch"] == 2


def test_resume_mid_epoch(whole, tmp_path):
    root = tmp_path / "run"
    rec = _Batches(kill_at=2)
    m, tr = _objects(root, callbacks=[rec], every=2)
    with pytest.raises(_Killed):
        tr.fit(m)
    first = _snapshot(m, tr)
    assert first["losses"] == whole["losses"][:2]  # (flushed before the snapshot of step 2)
    assert [p.name for p in (root / "checkpoints").iterdir()] == ["last.ckpt"]  # no epoch=... file from a step save
    ck = _load(root / "checkpoints" / "last.ckpt")
    assert ck["epoch"] == 0 and ck["global_step"] == 2
    assert ck["resume"]["epoch"] == 0 and ck["resume"]["batches_done"] == 2 and ck["resume"]["history_len"] == 2
    assert len((root / "metrics.jsonl").read_text().splitlines()) == 2
    rec2 = _Batches()
    m2, tr2 = _objects(root, callbacks=[rec2], every=2, seed_weights=False)
    tr2.fit(m2, ckpt_path=root / "checkpoints" / "last.ckpt")
    resumed = _snapshot(m2, tr2)
    _assert_same_run(whole, resumed, first)
    assert rec2.seen[0] == whole["batches"][2] and rec2.seen[0][:2] == (0, 2)  # its first trained batch: A's third
    assert rec2.seen == whole["batches"][2:]
    assert len((root / "metrics.jsonl").read_text().splitlines()) == 6


def _write_class_folders(root):
    rate, frames = 8000, 1200
    for split in ("train", "valid"):
        for ci, context in enumerate(("ballet", "salsa")):
            d = root / split / context
            d.mkdir(parents=True)
            for j in range(3):
                t = np.arange(frames) / rate
                y = 0.6 * np.sin(2 * np.pi * (220 + 110 * ci + 30 * j) * t) + 0.3 * np.sin(2 * np.pi * 50 * (j + 1) * t)
                with wave.open(str(d / f"c{j}.wav"), "wb") as w:
                    w.setnchannels(1)
                    w.setsampwidth(2)
                    w.setframerate(rate)
                    w.writeframes((y * 32767).round().astype("<i2").tobytes())


def test_label_dropout_masks_continue(tmp_path, monkeypatch):
    """Masks only: whether labelled training is bit-reproducible at this shape has not been measured."""
    import movenet_amd.wavenet as W
    monkeypatch.setattr(W, "MAX_AUDIO_FRAMES", 2000)  # (the length every clip is resampled to)
    monkeypatch.setattr(W, "MAX_VIDEO_FRAMES", 2)      # (... and the video up-sampler's kernel follows the two)
    _write_class_folders(tmp_path / "data")
    torch.manual_seed(1234)  # (Dance2Music seeds the dropout generator from torch's initial seed)

    def recorded(m):
        masks, inner = [], m.model.global_dropout_mask

        def mask(batch):
            out = inner(batch)
            masks.append(out.tolist())
            return out
        m.model.global_dropout_mask = mask
        return masks

    over = dict(dataset=str(tmp_path / "data"), use_global=True, global_dropout=0.5, num_workers=0, val_num_workers=0,
                seed_weights=False)
    m, tr = _objects(tmp_path / "whole", **over)
    assert m.global_classes == ["ballet", "salsa"]
    a = recorded(m)
    tr.fit(m)
    assert len(a) == 6 and a[:3] != a[3:]  # (else a generator that starts over would pass too)
    m1, tr1 = _objects(tmp_path / "run", max_epochs=1, **over)
    b = recorded(m1)
    tr1.fit(m1)
    m2, tr2 = _objects(tmp_path / "run", **over)
    b2 = recorded(m2)
    tr2.fit(m2, ckpt_path=tmp_path / "run" / "checkpoints" / "last.ckpt")
    assert len(b) == 3 and len(b2) == 3 and b + b2 == a
    assert _load(tmp_path / "run" / "checkpoints" / "last.ckpt")["global_classes"] == ["ballet", "salsa"]


def test_fine_tune_from_pretrained_model_path(whole, tmp_path):
    from movenet_amd.checkpoint import load_into
    from movenet_amd.config import ModelConfig, TrainingConfig
    from movenet_amd.pytorch_lightning_trainer import Dance2Music, train_model
    from movenet_amd.wavenet import WaveNet
    path = whole["root"] / "checkpoints" / "last.ckpt"
    assert max(_load(path)["optimizer_states"][0]["state"]["flat"]["steps"]) == 6
    cfg = TrainingConfig(model_config=ModelConfig(**SHAPE), batch_size=2, val_batch_size=2, n_epochs=1, use_video=False,
                         optimizer="AdamW", learning_rate=3e-3, weight_decay=0.01, model_output_path=tmp_path / "tuned",
                         scheduler="OneCycleLR", ema_decay=0.9, pretrained_model_path=path)
    tr = train_model(SPEC, cfg, limit_train_batches=1)
    assert len(tr.history) == 1 and tr.history[0]["step"] == 0 and tr.history[0]["epoch"] == 0
    assert sorted(set(tr.optimizer._steps)) == [0, 1] and tr.optimizer.ema_updates == 1  # a fresh optimizer: not 6 / 7
    assert tr.optimizer.state_dict()["param_groups"][0]["lr"] != whole["lr"]               # ... and a fresh schedule
    # the loss of step 0 is the file's weights' loss on the run's first batch
    loader = Dance2Music(SPEC, cfg).to(DEV)._loader(True)
    loader.set_epoch(0)
    batch = next(iter(loader))
    losses = []
    for pretrained in (True, False):
        fresh = WaveNet(**SHAPE)
        if pretrained:
            load_into(fresh, path)
        else:
            fresh.load_state_dict(make_state_dict(4, 2, 64, 64, 64, seed=5))  # (what run A started from)
        fresh.to(DEV).train()
        loss, _, _ = fresh(batch.audio.to(DEV), None, return_loss=True)
        losses.append(float(loss.detach()))
    print(f"step 0 train_loss {tr.history[0]['train_loss']!r}, file's weights {losses[0]!r}, untrained {losses[1]!r}")
    assert tr.history[0]["train_loss"] == losses[0]
    assert whole["losses"][0] == losses[1] and losses[0] != losses[1]


def test_resume_bf16(tmp_path):
    """Two uninterrupted bf16 runs first: if they are ``torch.equal`` so must the resumed run be; if not, the resumed
    run may differ from run A by no more than those two differ from each other (never a bound tuned on the resumed
    run).  Observed on an MI355X: the two uninterrupted runs are ``torch.equal`` (spread 0), so the first branch runs,
    and the resumed run is ``torch.equal`` to them."""
    a1 = _uninterrupted(tmp_path / "a1", precision="bf16")
    a2 = _uninterrupted(tmp_path / "a2", precision="bf16")
    first, resumed = _epoch_boundary(tmp_path / "run", precision="bf16")

    def spread(x, y):
        return max(max(float((x["state"][k].double() - y["state"][k].double()).abs().max()) for k in x["state"]),
                   max(float((x["buffers"][k].double() - y["buffers"][k].double()).abs().max()) for k in x["buffers"]))

    reproducible = (all(torch.equal(a1["state"][k], a2["state"][k]) for k in a1["state"])
                    and all(torch.equal(a1["buffers"][k], a2["buffers"][k]) for k in a1["buffers"])
                    and a1["losses"] == a2["losses"])
    between, to_resumed = spread(a1, a2), spread(a1, resumed)
    print(f"bf16: two uninterrupted runs {'are torch.equal' if reproducible else 'differ'} (spread {between:.3e}); "
          f"resumed run against run A: {to_resumed:.3e}")
    assert resumed["steps"] == a1["steps"] and resumed["ema_updates"] == a1["ema_updates"] == 6
    assert resumed["lr"] == a1["lr"] and len(first["losses"]) == len(resumed["losses"]) == 3
    if reproducible:
        _assert_same_run(a1, resumed, first)
    else:
        assert to_resumed <= between
        loss_spread = max(abs(x - y) for x, y in zip(a1["losses"], a2["losses"]))
        assert max(abs(x - y) for x, y in zip(a1["losses"], first["losses"] + resumed["losses"])) <= loss_spread
