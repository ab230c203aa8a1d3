"""CPU: the host side of the "model" sampling rule -- the trainer's flag and config field, the model property, and
the C ABI's argument check, none of which needs a device."""
import json

import pytest

from movenet_amd import _native as N
from movenet_amd.config import ModelConfig, TrainingConfig, arg_parser, config_from_args


def test_flag_default_and_choices():
    assert arg_parser().parse_args([]).generate_sampling == "reference"
    assert arg_parser().parse_args(["--generate_sampling", "model"]).generate_sampling == "model"
    with pytest.raises(SystemExit):
        arg_parser().parse_args(["--generate_sampling", "top-k"])
    assert TrainingConfig().generate_sampling == "reference"


def test_config_from_args_copies_the_rule():
    base = "--dataset synthetic://clips=4,frames=100 --use_video 0".split()
    assert config_from_args(arg_parser().parse_args(base)).generate_sampling == "reference"
    c = config_from_args(arg_parser().parse_args(base + ["--generate_sampling", "model"]))
    assert c.generate_sampling == "model"
    assert TrainingConfig.from_json(c.to_json()).generate_sampling == "model"


def test_json_without_the_field_loads_with_the_default():
    d = json.loads(TrainingConfig(generate_sampling="model", batch_size=5).to_json())
    assert d.pop("generate_sampling") == "model"
    back = TrainingConfig.from_json(json.dumps(d))  # what a run before the field existed wrote
    assert back.generate_sampling == "reference" and back.batch_size == 5


def test_dance2music_hands_the_rule_to_the_model():
    from movenet_amd.pytorch_lightning_trainer import Dance2Music
    mc = ModelConfig(2, 2, 16, 8, 8)
    m = Dance2Music("synthetic://clips=2,frames=40", TrainingConfig(model_config=mc, use_video=False,
                                                                    generate_sampling="model"))
    assert m.model.generate_sampling == "model"
    assert Dance2Music("synthetic://clips=2,frames=40",
                       TrainingConfig(model_config=mc, use_video=False)).model.generate_sampling == "reference"
    with pytest.raises(ValueError, match="sampling"):
        Dance2Music("synthetic://clips=2,frames=40", TrainingConfig(model_config=mc, use_video=False,
                                                                    generate_sampling="nucleus"))
    with pytest.raises(ValueError, match="sampling"):
        m.model.generate_sampling = "top-k"
    assert m.model.generate_sampling == "model"


def test_sampling_rule_names():
    assert (N.SAMPLE_REFERENCE, N.SAMPLE_MODEL) == (0, 1)
    assert N.sampling_rule("reference") == N.SAMPLE_REFERENCE and N.sampling_rule("model") == N.SAMPLE_MODEL
    for bad in ("", "Model", None, 1):
        with pytest.raises(ValueError, match="sampling"):
            N.sampling_rule(bad)


def test_generate_ex_refuses_an_unknown_rule_before_any_launch():
    lib = N.lib()
    d2 = N.make_dims(10, 3, 256, 64, 64)
    args = (d2, N.GEN_STREAM, None, None, None, 1, 10, 10, 1, 0, 5, 1.0, 0, None, None, 0, None)
    for bad in (2, -1):
        assert lib.mvn_generate_ex(*args, bad, None) == N.MVN_ERR_BAD_ARG
        assert "sampling" in N.last_error()
        with pytest.raises(ValueError):
            N.check(N.MVN_ERR_BAD_ARG, "mvn_generate_ex")
    # both known rules get past that check, to the NULL buffers
    for ok in (N.SAMPLE_REFERENCE, N.SAMPLE_MODEL):
        assert lib.mvn_generate_ex(*args, ok, None) == N.MVN_ERR_BAD_ARG
        assert "sampling" not in N.last_error() and "bad argument" in N.last_error()
