"""Host: the trainer's complete checkpoints and what ``Trainer.fit(ckpt_path=...)`` refuses, with no GPU.

1. ``checkpoint.training_checkpoint`` writes exactly the documented keys, into a file that loads under
   ``weights_only=True``.
2. ``--resume_from auto`` resolves to ``last.ckpt`` when there is one and to a fresh run when there is none.
3. Every refusal of ``fit(ckpt_path=...)`` is a ValueError naming the file and the field, raised before the device is
   touched (the tests run where there is none: a file that passes the checks gets as far as the trainer's "no CPU path").
4. ``write_checkpoint`` is atomic: a ``torch.save`` that fails part-way leaves the previous ``last.ckpt`` intact.
5. The label-dropout generator's state round-trips through a file.
6. ``synthesize`` / ``evaluate`` take the model's shape from ``hyper_parameters``, else from the defaults.
7. ``--pretrained_model_path`` with ``--resume_from``, or with other class names than the run's, is a ValueError.
"""
import pytest
import torch

from movenet_amd import checkpoint
from movenet_amd.config import ModelConfig, TrainingConfig, arg_parser, config_from_args

SPEC = "synthetic://clips=6,frames=600,seed=5"
SHAPE = dict(layer_size=2, stack_size=2, input_channels=64, residual_channels=16, skip_channels=16)

TOP_KEYS = {"epoch", "global_step", "state_dict", "optimizer_states", "lr_schedulers", "hyper_parameters", "resume"}
HYPER_KEYS = {"layer_size", "stack_size", "input_channels", "residual_channels", "skip_channels", "precision",
              "bf16_video", "loss_rule", "optimizer", "scheduler", "accumulation_steps", "batch_size", "world_size",
              "dataset"}
RESUME_KEYS = {"epoch", "batches_done", "global_dropout_generator", "torch_rng", "history_len"}


def _module(tmp_path, **over):
    from movenet_amd.pytorch_lightning_trainer import Dance2Music
    kw = dict(model_config=ModelConfig(**SHAPE), batch_size=2, val_batch_size=2, n_epochs=2, use_video=False,
              optimizer="AdamW", learning_rate=3e-3, scheduler="OneCycleLR", model_output_path=tmp_path / "run")
    return Dance2Music(SPEC, TrainingConfig(**{**kw, **over}))


def _trainer(tmp_path, max_epochs=2, **kw):
    from movenet_amd.pytorch_lightning_trainer import Trainer
    return Trainer(max_epochs=max_epochs, default_root_dir=tmp_path / "run", device="cpu", **kw)


def _written(tmp_path, name="last.ckpt", next_epoch=1, batches_done=0, module=None, **hyper_over):
    """A checkpoint of one CPU step of ``module`` (torch's AdamW: the fused one steps on the GPU only), through the
    writer the trainer uses."""
    m = module if module is not None else _module(tmp_path)
    cfg = m.configure_optimizers()
    opt, sched = cfg["optimizer"], cfg["lr_scheduler"]["scheduler"]
    for p in m.model.parameters():
        p.grad = torch.full_like(p, 0.01)
    opt.step()
    sched.step()
    hyper = {**checkpoint.hyper_parameters(m.config, SPEC, 32, False, 1, 1), **hyper_over}
    obj = checkpoint.training_checkpoint(m, opt, sched, epoch=0, global_step=3, next_epoch=next_epoch,
                                         batches_done=batches_done, hyper=hyper, history_len=3)
    path = tmp_path / name
    checkpoint.write_checkpoint(obj, path)
    return path, m, opt, sched


def test_written_checkpoint_has_the_documented_keys_and_loads_weights_only(tmp_path):
    path, m, opt, sched = _written(tmp_path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert set(ck) == TOP_KEYS  # (no labels, no average, no mel, no pre-emphasis: their keys are absent)
    assert set(ck["hyper_parameters"]) == HYPER_KEYS and set(ck["resume"]) == RESUME_KEYS
    assert all(type(v) in (int, float, str, bool) for v in ck["hyper_parameters"].values())
    assert ck["hyper_parameters"] == {**SHAPE, "precision": 32, "bf16_video": False, "loss_rule": "reference",
                                      "optimizer": "AdamW", "scheduler": "OneCycleLR", "accumulation_steps": 1,
                                      "batch_size": 2, "world_size": 1, "dataset": SPEC}
    assert ck["epoch"] == 0 and ck["global_step"] == 3
    assert ck["resume"]["epoch"] == 1 and ck["resume"]["batches_done"] == 0 and ck["resume"]["history_len"] == 3
    assert ck["resume"]["torch_rng"].dtype == torch.uint8 and ck["resume"]["global_dropout_generator"].dtype == torch.uint8
    want = m.model.state_dict()
    assert sorted(ck["state_dict"]) == sorted(f"model.{k}" for k in want)
    assert all(torch.equal(ck["state_dict"][f"model.{k}"], v) for k, v in want.items())
    # the optimizer's and the scheduler's own state dicts, loadable into fresh ones
    assert len(ck["optimizer_states"]) == 1 and len(ck["lr_schedulers"]) == 1
    assert set(ck["optimizer_states"][0]) == {"state", "param_groups"}
    assert ck["optimizer_states"][0]["param_groups"][0]["lr"] == opt.param_groups[0]["lr"]
    assert ck["lr_schedulers"][0]["last_epoch"] == sched.last_epoch == 1
    fresh = _module(tmp_path).configure_optimizers()
    fresh["optimizer"].load_state_dict(ck["optimizer_states"][0])
    fresh["lr_scheduler"]["scheduler"].load_state_dict(ck["lr_schedulers"][0])
    assert fresh["optimizer"].param_groups[0]["lr"] == opt.param_groups[0]["lr"]
    a, b = opt.state_dict()["state"], fresh["optimizer"].state_dict()["state"]
    assert a.keys() == b.keys() and all(torch.equal(a[k]["exp_avg_sq"], b[k]["exp_avg_sq"]) for k in a)
    # a run with labels and pre-emphasis keeps the keys it wrote before
    labelled = _module(tmp_path, use_global=True, preemphasis=0.5)
    path, _, _, _ = _written(tmp_path, "labelled.ckpt", module=labelled)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert set(ck) == TOP_KEYS | {"global_classes", "preemphasis"}
    assert ck["global_classes"] == ["synthetic"] and ck["preemphasis"] == 0.5
    # no scheduler: an empty list, and "" in the record
    m = _module(tmp_path, scheduler=None)
    opt = m.configure_optimizers()["optimizer"]
    obj = checkpoint.training_checkpoint(m, opt, None, epoch=0, global_step=0, next_epoch=1, batches_done=0,
                                         hyper=checkpoint.hyper_parameters(m.config, SPEC), history_len=0)
    assert obj["lr_schedulers"] == [] and obj["hyper_parameters"]["scheduler"] == ""


def test_resume_from_auto(tmp_path):
    cfg = config_from_args(arg_parser().parse_args(["--dataset", SPEC, "--resume_from", "auto",
                                                    "--checkpoint_every_n_steps", "50",
                                                    "--model_output_path", str(tmp_path / "run")]))
    assert cfg.resume_from == "auto" and cfg.checkpoint_every_n_steps == 50
    off = config_from_args(arg_parser().parse_args(["--dataset", SPEC]))
    assert off.resume_from is None and off.checkpoint_every_n_steps == 0
    assert TrainingConfig().resume_from is None and TrainingConfig().checkpoint_every_n_steps == 0
    assert TrainingConfig.from_json(cfg.to_json()).resume_from == "auto"
    assert checkpoint.resolve_resume("auto", cfg.model_output_path) is None  # no file: a fresh run
    assert checkpoint.resolve_resume(None, cfg.model_output_path) is None
    last = tmp_path / "run" / "checkpoints" / "last.ckpt"
    last.parent.mkdir(parents=True)
    last.write_bytes(b"x")
    assert checkpoint.resolve_resume("auto", cfg.model_output_path) == last
    assert checkpoint.resolve_resume(str(last), tmp_path / "elsewhere") == last
    with pytest.raises(FileNotFoundError, match="nowhere.ckpt"):
        checkpoint.resolve_resume(str(tmp_path / "nowhere.ckpt"), cfg.model_output_path)


@pytest.mark.parametrize("field,run_over,trainer_over", [
    ("layer_size", dict(model_config=ModelConfig(**{**SHAPE, "layer_size": 3})), {}),
    ("skip_channels", dict(model_config=ModelConfig(**{**SHAPE, "skip_channels": 32})), {}),
    ("optimizer", dict(optimizer="Adam"), {}),
    ("scheduler", dict(scheduler="StepLR"), {}),
    ("scheduler", dict(scheduler=None), {}),
    ("precision", {}, dict(precision="bf16")),
    ("accumulation_steps", {}, dict(accumulate_grad_batches=2)),
    ("batch_size", dict(batch_size=3), {}),
])
def test_fit_refuses_a_file_of_another_run(tmp_path, field, run_over, trainer_over):
    path, _, _, _ = _written(tmp_path)
    if field == "precision":  # (the bf16 layer kernels take C = K = 64 only: the file gets that shape too)
        wide = dict(model_config=ModelConfig(**{**SHAPE, "residual_channels": 64, "skip_channels": 64}))
        path, _, _, _ = _written(tmp_path, module=_module(tmp_path, **wide))
        run_over = wide
    with pytest.raises(ValueError) as e:
        _trainer(tmp_path, **trainer_over).fit(_module(tmp_path, **run_over), ckpt_path=path)
    assert str(path) in str(e.value) and f"hyper_parameters['{field}']" in str(e.value)


def test_fit_refuses_another_world_size(tmp_path):
    path, _, _, _ = _written(tmp_path, world_size=8)
    with pytest.raises(ValueError, match=r"hyper_parameters\['world_size'\] is 8, but this run has 1") as e:
        _trainer(tmp_path).fit(_module(tmp_path), ckpt_path=path)
    assert str(path) in str(e.value)


def test_fit_refuses_files_that_cannot_be_resumed(tmp_path):
    m = _module(tmp_path)
    # an older checkpoint: weights, no optimizer state
    old = tmp_path / "old.ckpt"
    torch.save({"epoch": 0, "global_step": 3,
                "state_dict": {f"model.{k}": v for k, v in m.model.state_dict().items()}}, old)
    with pytest.raises(ValueError, match="no 'optimizer_states'.*--pretrained_model_path") as e:
        _trainer(tmp_path).fit(m, ckpt_path=old)
    assert str(old) in str(e.value)
    # nothing left to train
    path, _, _, _ = _written(tmp_path, next_epoch=2)
    with pytest.raises(ValueError, match=r"resume\['epoch'\] is 2.*max_epochs = 2") as e:
        _trainer(tmp_path).fit(_module(tmp_path), ckpt_path=path)
    assert str(path) in str(e.value)
    with pytest.raises(ValueError, match=r"resume\['epoch'\] is 2.*max_epochs = 1"):
        _trainer(tmp_path, max_epochs=1).fit(_module(tmp_path), ckpt_path=path)
    # the run averages its weights, the file holds no average
    path, _, _, _ = _written(tmp_path)
    with pytest.raises(ValueError, match=r"optimizer_states\[0\]\['state'\]\['flat'\] holds no 'ema'.*--ema_decay") as e:
        _trainer(tmp_path).fit(_module(tmp_path, ema_decay=0.9), ckpt_path=path)
    assert str(path) in str(e.value)
    # other class names than the run's
    with pytest.raises(ValueError, match="global_classes") as e:
        _trainer(tmp_path).fit(_module(tmp_path, use_global=True), ckpt_path=path)
    assert str(path) in str(e.value)


def test_a_fitting_file_passes_the_checks_before_the_device_is_asked_for(tmp_path):
    """The checks need no device and come first: a file that passes them gets as far as the trainer's refusal of
    ``device="cpu"``, a file that fails them (above) never does."""
    path, _, _, _ = _written(tmp_path)
    with pytest.raises(RuntimeError, match="MI355X devices only"):
        _trainer(tmp_path).fit(_module(tmp_path), ckpt_path=path)
    mid, _, _, _ = _written(tmp_path, "mid.ckpt", next_epoch=0, batches_done=2)
    with pytest.raises(RuntimeError, match="MI355X devices only"):
        _trainer(tmp_path).fit(_module(tmp_path), ckpt_path=mid)


def test_last_ckpt_write_is_atomic(tmp_path, monkeypatch):
    path, _, _, _ = _written(tmp_path)
    before = path.read_bytes()
    real_save = torch.save

    def failing_save(obj, f, *a, **k):
        with open(f, "wb") as fh:  # part of a file, then the failure
            fh.write(b"PK\x03\x04 half a checkpoint")
        raise OSError("disk full")

    monkeypatch.setattr(torch, "save", failing_save)
    with pytest.raises(OSError, match="disk full"):
        checkpoint.write_checkpoint({"epoch": 7}, path)
    monkeypatch.setattr(torch, "save", real_save)
    assert path.read_bytes() == before
    assert torch.load(path, map_location="cpu", weights_only=True)["global_step"] == 3
    assert sorted(p.name for p in tmp_path.iterdir() if p.is_file()) == ["last.ckpt"]  # no temporary file left behind
    checkpoint.write_checkpoint({"epoch": 7}, path)  # and a save that succeeds replaces it
    assert torch.load(path, map_location="cpu", weights_only=True) == {"epoch": 7}
    assert sorted(p.name for p in tmp_path.iterdir() if p.is_file()) == ["last.ckpt"]


def test_global_dropout_generator_state_round_trips(tmp_path):
    m = _module(tmp_path, use_global=True, global_dropout=0.5)
    g = m.model.global_dropout_generator
    torch.rand(7, generator=g)  # (somewhere inside its stream)
    path, _, _, _ = _written(tmp_path, module=m)
    want = [torch.rand(3, generator=g) for _ in range(32)]
    fresh = _module(tmp_path, use_global=True, global_dropout=0.5)
    torch.rand(100, generator=fresh.model.global_dropout_generator)
    fresh.model.global_dropout_generator.set_state(
        torch.load(path, map_location="cpu", weights_only=True)["resume"]["global_dropout_generator"])
    got = [torch.rand(3, generator=fresh.model.global_dropout_generator) for _ in range(32)]
    assert all(torch.equal(a, b) for a, b in zip(want, got))
    assert len({tuple(t.tolist()) for t in want}) == 32


@pytest.mark.parametrize("cli", ["synthesize", "evaluate"])
def test_cli_reads_the_shape_from_the_file(tmp_path, cli):
    import importlib
    from movenet_amd.synthesize import load_model
    mod = importlib.import_module(f"movenet_amd.{cli}")
    path, m, _, _ = _written(tmp_path)
    rest = ["--out", str(tmp_path / "o"), "--seconds", "0.01"] if cli == "synthesize" else ["--wavs", str(tmp_path)]
    errors = []

    def fail(message):
        errors.append(message)
        raise SystemExit(2)

    args = mod.build_parser().parse_args(["--checkpoint", str(path)] + rest)
    assert [getattr(args, k) for k in SHAPE] == [None] * 5
    model, rec, names = load_model(args, fail)
    assert {k: getattr(args, k) for k in SHAPE} == SHAPE and rec is None and names == []
    assert all(torch.equal(v, m.model.state_dict()[k]) for k, v in model.state_dict().items())
    # a flag that contradicts the record: the error it always was
    args = mod.build_parser().parse_args(["--checkpoint", str(path), "--residual_channels", "32"] + rest)
    with pytest.raises(SystemExit):
        load_model(args, fail)
    assert "does not fit --input_channels 64 --residual_channels 32 --skip_channels 16" in errors[-1]
    # a file without the record: the defaults
    plain = tmp_path / "plain.ckpt"
    torch.save({"state_dict": {f"model.{k}": v for k, v in m.model.state_dict().items()}}, plain)
    args = mod.build_parser().parse_args(["--checkpoint", str(plain)] + rest)
    with pytest.raises(SystemExit):
        load_model(args, fail)
    assert (args.input_channels, args.residual_channels, args.skip_channels, args.layer_size, args.stack_size) == \
        (256, 64, 64, 10, 3)
    assert "does not fit --input_channels 256 --residual_channels 64 --skip_channels 64 --layer_size 10 " \
           "--stack_size 3" in errors[-1]
    args = mod.build_parser().parse_args(["--checkpoint", str(plain)] + rest
                                         + [s for k, v in SHAPE.items() for s in (f"--{k}", str(v))])
    assert load_model(args, fail)[0].receptive_fields == m.model.receptive_fields


def test_pretrained_model_path_refusals(tmp_path):
    from movenet_amd.pytorch_lightning_trainer import train_model
    path, m, _, _ = _written(tmp_path)
    kw = dict(model_config=ModelConfig(**SHAPE), batch_size=2, use_video=False, model_output_path=tmp_path / "run",
              pretrained_model_path=path)
    with pytest.raises(ValueError, match="--pretrained_model_path.*--resume_from"):
        train_model(SPEC, TrainingConfig(**kw, resume_from="auto"))
    with pytest.raises(ValueError, match="global_classes") as e:
        train_model(SPEC, TrainingConfig(**kw, use_global=True))
    assert str(path) in str(e.value)
