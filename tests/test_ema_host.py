"""CPU: the host side of the weights' exponential moving average (``--ema_decay``): the decay schedule, the refusals
of ``mvn_adamw_ema_step`` (no device needed: they come before any launch), the flags, and reading the averaged weights
out of a checkpoint file."""
import ctypes

import pytest
import torch

from movenet_amd import _native as N


@pytest.mark.parametrize("decay", [0.9, 0.999])
def test_ema_decay_at(decay):
    from movenet_amd.optim import ema_decay_at
    for t in (0, 1, 7, 100, 10 ** 6):
        assert ema_decay_at(decay, t, False) == decay
    assert ema_decay_at(decay, 0, True) == 0.1
    assert ema_decay_at(decay, 1, True) == 2.0 / 11.0
    # the ramp (1 + t) / (10 + t) grows with t: from the first t at which it reaches `decay`, the decay is `decay`
    first = next(t for t in range(10 ** 5) if (1.0 + t) / (10.0 + t) >= decay)
    assert first == {0.9: 80, 0.999: 8990}[decay]  # (1 + t) / (10 + t) >= d  <=>  t >= (10 d - 1) / (1 - d)
    for t in range(first):
        assert ema_decay_at(decay, t, True) == (1.0 + t) / (10.0 + t) < decay
    for t in (first, first + 1, 10 * first, 10 ** 7):
        assert ema_decay_at(decay, t, True) == decay


def _call(**over):
    """mvn_adamw_ema_step on pointers that are never dereferenced (every case is refused before a launch)."""
    fake = ctypes.c_void_p(0x1000)
    skips = (ctypes.c_size_t * 10)(*range(10))
    kw = dict(param=fake, grad=fake, exp_avg=fake, exp_avg_sq=fake, ema=fake, n=16, lr=1e-3, beta1=0.9, beta2=0.999,
              eps=1e-8, weight_decay=0.0, step=1, decoupled=1, ema_weight=0.1, skip_ranges=skips, n_skip=0, stream=None)
    kw.update(over)
    return N.lib().mvn_adamw_ema_step(*kw.values())


@pytest.mark.parametrize("over", [dict(ema=None), dict(ema_weight=0.0), dict(ema_weight=1.5),
                                  dict(ema_weight=float("nan")), dict(step=0), dict(n_skip=5)],
                         ids=["null-ema", "weight-0", "weight-1.5", "weight-nan", "step-0", "five-skips"])
def test_adamw_ema_step_refusals(over):
    assert _call(**over) == N.MVN_ERR_BAD_ARG
    assert "mvn_adamw_ema_step" in N.last_error()
    with pytest.raises(ValueError):
        N.check(N.MVN_ERR_BAD_ARG, "mvn_adamw_ema_step")


def test_adamw_ema_step_nothing_to_do():
    assert _call(n=0) == N.MVN_OK                    # (no launch: nothing is dereferenced)
    assert _call(n=0, ema_weight=1.0) == N.MVN_OK    # 1 is inside (0, 1]
    assert _call(n=0, ema_weight=-0.25) == N.MVN_ERR_BAD_ARG  # the refusals come first


def test_flags_and_config():
    from movenet_amd.config import TrainingConfig, arg_parser, config_from_args
    args = arg_parser().parse_args(["--dataset", "synthetic://clips=2,frames=100"])
    assert args.ema_decay == 0.0 and args.ema_warmup == 1
    cfg = config_from_args(args)
    assert cfg.ema_decay == 0.0 and cfg.ema_warmup is True
    assert TrainingConfig().ema_decay == 0.0 and TrainingConfig().ema_warmup is True
    args = arg_parser().parse_args(["--dataset", "x", "--ema_decay", "0.999", "--ema_warmup", "0"])
    cfg = config_from_args(args)
    assert cfg.ema_decay == 0.999 and cfg.ema_warmup is False
    again = TrainingConfig.from_json(cfg.to_json())
    assert again.ema_decay == 0.999 and again.ema_warmup is False
    # a JSON written before the fields existed loads with the average off
    d = {k: v for k, v in cfg.to_dict().items() if not k.startswith("ema_")}
    import json
    old = TrainingConfig.from_json(json.dumps(d, default=str))
    assert old.ema_decay == 0.0 and old.ema_warmup is True


def test_ema_needs_the_flat_optimizer():
    """--ema_decay with an optimizer that has no fused step (here: any, on the CPU) is refused by name."""
    from movenet_amd.config import ModelConfig, TrainingConfig
    from movenet_amd.pytorch_lightning_trainer import Dance2Music
    mc = ModelConfig(layer_size=2, stack_size=2, input_channels=64, residual_channels=16, skip_channels=16)
    for opt in ("SGD", "AdamW"):
        cfg = TrainingConfig(model_config=mc, use_video=False, optimizer=opt, scheduler=None, ema_decay=0.9)
        with pytest.raises(ValueError, match="--ema_decay"):
            Dance2Music("synthetic://clips=2,frames=100", cfg).configure_optimizers()
    cfg = TrainingConfig(model_config=mc, use_video=False, optimizer="SGD", scheduler=None)
    m = Dance2Music("synthetic://clips=2,frames=100", cfg)
    assert isinstance(m.configure_optimizers()["optimizer"], torch.optim.SGD) and m.ema_optimizer is None


def test_checkpoint_reading(tmp_path):
    from movenet_amd.checkpoint import load_into, load_state_dict_file
    lin = torch.nn.Linear(3, 2)
    raw = {k: v.detach().clone() for k, v in lin.state_dict().items()}
    avg = {k: v + 1.0 for k, v in raw.items()}
    with_ema, without = tmp_path / "ema.ckpt", tmp_path / "plain.ckpt"
    torch.save({"epoch": 0, "global_step": 3, "state_dict": {f"model.{k}": v for k, v in raw.items()},
                "ema_state_dict": {f"model.{k}": v for k, v in avg.items()}, "ema_decay": 0.9, "ema_updates": 3},
               with_ema)
    torch.save({"epoch": 0, "global_step": 3, "state_dict": {f"model.{k}": v for k, v in raw.items()}}, without)
    for path in (with_ema, without):  # the default read: what it was
        got = load_state_dict_file(path)
        assert list(got) == list(raw) and all(torch.equal(got[k], raw[k]) for k in raw)
        assert list(load_state_dict_file(path, ema=False)) == list(raw)
    got = load_state_dict_file(with_ema, ema=True)
    assert list(got) == list(avg) and all(torch.equal(got[k], avg[k]) for k in avg)  # prefixes stripped
    load_into(lin, with_ema, ema=True)
    assert all(torch.equal(v, avg[k]) for k, v in lin.state_dict().items())
    load_into(lin, with_ema)
    assert all(torch.equal(v, raw[k]) for k, v in lin.state_dict().items())
    with pytest.raises(ValueError, match="ema_state_dict"):
        load_state_dict_file(without, ema=True)
    with pytest.raises(ValueError, match="ema_state_dict"):
        load_into(lin, without, ema=True)
    bare = tmp_path / "model.pth"  # the legacy trainer's bare state_dict
    torch.save(raw, bare)
    assert list(load_state_dict_file(bare)) == list(raw)
    with pytest.raises(ValueError, match="ema_state_dict"):
        load_state_dict_file(bare, ema=True)
