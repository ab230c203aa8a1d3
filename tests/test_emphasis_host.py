"""CPU: the host side of pre-emphasis / de-emphasis -- the flag and the config field, the checkpoint's record, the model's
validated property, the state ``ops.pcm16_chunk`` insists on, ``synthesize``'s rule for flag against record, and the
float64 reference's own round trip."""
import json
import math

import pytest
import torch

import emphasis_reference as R
from movenet_amd import checkpoint, ops
from movenet_amd import synthesize as S
from movenet_amd.config import TrainingConfig, arg_parser, config_from_args
from movenet_amd.wavenet import WaveNet

TINY = dict(layer_size=2, stack_size=2, input_channels=64, residual_channels=16, skip_channels=16)
TINY_FLAGS = [x for k, v in TINY.items() for x in (f"--{k}", str(v))]


def test_flag_parses_and_defaults_to_zero():
    base = ["--dataset", "x"]
    assert config_from_args(arg_parser().parse_args(base)).preemphasis == 0.0
    cfg = config_from_args(arg_parser().parse_args(base + ["--preemphasis", "0.97"]))
    assert cfg.preemphasis == 0.97
    assert TrainingConfig.from_json(cfg.to_json()).preemphasis == 0.97


def test_a_config_without_the_field_loads():
    old = json.loads(TrainingConfig().to_json())
    del old["preemphasis"]
    assert TrainingConfig.from_json(json.dumps(old)).preemphasis == 0.0


def test_model_property_is_validated_and_not_in_the_state_dict():
    m = WaveNet(**TINY)
    assert m.preemphasis == 0.0
    keys = set(m.state_dict())
    m.preemphasis = 0.97
    assert m.preemphasis == 0.97 and set(m.state_dict()) == keys
    for bad in (-0.1, 1.0, 1.5, math.nan, 1.0 - 1e-12, "0.5", True):   # (1 - 1e-12 is 1.0 as a float32)
        with pytest.raises(ValueError, match="preemphasis"):
            m.preemphasis = bad
    assert m.preemphasis == 0.97
    m.preemphasis = 0
    assert m.preemphasis == 0.0


def _checkpoint(tmp_path, model, name="m.ckpt", **records):
    path = tmp_path / name
    torch.save({"epoch": 0, **records, "state_dict": {f"model.{k}": v for k, v in model.state_dict().items()}}, path)
    return str(path)


def test_checkpoint_record_round_trips_and_is_absent_at_zero(tmp_path):
    m = WaveNet(**TINY)
    assert checkpoint.preemphasis_record(m) == {}
    plain = _checkpoint(tmp_path, m, "plain.ckpt", **checkpoint.preemphasis_record(m))
    assert "preemphasis" not in torch.load(plain, weights_only=True)
    assert checkpoint.preemphasis_of(plain) == 0.0
    m.preemphasis = 0.97
    assert checkpoint.preemphasis_record(m) == {"preemphasis": 0.97}
    path = _checkpoint(tmp_path, m, **checkpoint.preemphasis_record(m))
    assert checkpoint.preemphasis_of(path) == 0.97
    fresh = WaveNet(**TINY)
    checkpoint.load_into(fresh, path)
    assert fresh.preemphasis == 0.97
    checkpoint.load_into(fresh, plain)   # a file without the record leaves the setting alone
    assert fresh.preemphasis == 0.97


def test_pcm16_chunk_needs_a_state_for_deemphasis():
    x = torch.zeros(2, 10, dtype=torch.int32)
    with pytest.raises(ValueError, match="state"):
        ops.pcm16_chunk(x, 0, 4, 64, deemphasis=0.5, state=None)
    for bad in (-0.5, 1.0, math.nan):
        with pytest.raises(ValueError, match="deemphasis"):
            ops.pcm16_chunk(x, 0, 4, 64, deemphasis=bad, state=torch.zeros(2, dtype=torch.float64))


def test_synthesize_flag_against_the_checkpoints_record(tmp_path, capsys):
    m = WaveNet(**TINY)
    recorded = _checkpoint(tmp_path, m, "recorded.ckpt", preemphasis=0.97)
    plain = _checkpoint(tmp_path, m, "plain.ckpt")

    def load(path, *flags):
        args = S.build_parser().parse_args(["--checkpoint", path, "--out", str(tmp_path / "o"), "--seconds", "0.01",
                                            *TINY_FLAGS, *flags])

        def fail(message):
            raise RuntimeError(message)
        return S.load_model(args, fail)[0]

    assert load(recorded).preemphasis == 0.97                         # no flag: the record
    assert load(recorded, "--preemphasis", "0.97").preemphasis == 0.97
    assert load(plain).preemphasis == 0.0
    assert load(plain, "--preemphasis", "0.9").preemphasis == 0.9      # no record: the flag stands
    with pytest.raises(RuntimeError, match="records preemphasis 0.97"):
        load(recorded, "--preemphasis", "0.5")
    with pytest.raises(RuntimeError, match="records preemphasis 0.97"):
        load(recorded, "--preemphasis", "0")
    assert load(recorded, "--preemphasis", "0.5", "--force_preemphasis", "1").preemphasis == 0.5
    with pytest.raises(RuntimeError, match=r"\[0, 1\)"):
        load(plain, "--preemphasis", "1.0")
    # ... and through main() it is the parser's error: exit status 2, the message on stderr, before any device is used
    with pytest.raises(SystemExit) as e:
        S.main(["--checkpoint", recorded, "--out", str(tmp_path / "o"), "--seconds", "0.01", *TINY_FLAGS,
                "--preemphasis", "0.5"])
    assert e.value.code == 2 and "records preemphasis 0.97" in capsys.readouterr().err


def test_reference_round_trip():
    assert R.self_check() <= 1e-12
