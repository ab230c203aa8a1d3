"""CPU: the bf16 training switch's host surface -- the --precision flag, train_model passing it to Trainer,
Trainer validating it -- and the new C entry points in the header and the binding."""
import os

import pytest

from movenet_amd import _native as N
from movenet_amd.config import ModelConfig, TrainingConfig, arg_parser

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_precision_flag_parses_with_default_32():
    assert arg_parser().parse_args([]).precision == 32
    assert arg_parser().parse_args(["--precision", "32"]).precision == 32
    assert arg_parser().parse_args(["--precision", "bf16"]).precision == "bf16"
    with pytest.raises(SystemExit):
        arg_parser().parse_args(["--precision", "16"])


def test_trainer_validates_precision():
    from movenet_amd.pytorch_lightning_trainer import Trainer
    assert Trainer(max_epochs=1).precision == 32
    assert Trainer(max_epochs=1, precision=32).precision == 32
    assert Trainer(max_epochs=1, precision="bf16").precision == "bf16"
    for p in (16, "16", "16-mixed"):
        with pytest.raises(NotImplementedError, match="loss scaling"):
            Trainer(max_epochs=1, precision=p)
    for p in (64, "fp32", "bf8"):
        with pytest.raises(ValueError):
            Trainer(max_epochs=1, precision=p)


def _config(tmp_path, use_video=False, C=64):
    mc = ModelConfig(layer_size=2, stack_size=2, input_channels=64, residual_channels=C, skip_channels=C)
    return TrainingConfig(model_config=mc, batch_size=2, val_batch_size=2, n_epochs=1, use_video=use_video,
                          model_output_path=tmp_path)


def test_train_model_passes_precision(tmp_path, monkeypatch):
    from movenet_amd import pytorch_lightning_trainer as T
    seen = []
    monkeypatch.setattr(T.Trainer, "fit", lambda self, model: seen.append(self.precision))
    T.train_model("synthetic://clips=2,frames=400", _config(tmp_path))
    T.train_model("synthetic://clips=2,frames=400", _config(tmp_path), precision="bf16")
    assert seen == [32, "bf16"]


def test_fit_refuses_bf16_with_video_or_other_channels(tmp_path):
    from movenet_amd.pytorch_lightning_trainer import Dance2Music, Trainer
    with pytest.raises(ValueError, match="audio-only"):
        Trainer(max_epochs=1, precision="bf16").fit(Dance2Music("synthetic://clips=2,frames=400",
                                                                _config(tmp_path, use_video=True)))
    with pytest.raises(ValueError, match="residual_channels = skip_channels = 64"):
        Trainer(max_epochs=1, precision="bf16").fit(Dance2Music("synthetic://clips=2,frames=400",
                                                                _config(tmp_path, C=16)))


def test_bf16_entry_points_declared_and_bound():
    with open(os.path.join(ROOT, "include", "movenet_hip.h")) as f:
        header = f.read()
    for name in ("mvn_forward_bf16", "mvn_backward_bf16"):
        assert f"int {name}(" in header and name in N.SIGNATURES
    assert N.SIGNATURES["mvn_forward_bf16"] == N.SIGNATURES["mvn_forward"]
    assert N.SIGNATURES["mvn_backward_bf16"] == N.SIGNATURES["mvn_backward"]
    assert "#define MVN_BWD_FORM_BF16 4" in header and N.BWD_FORM_BF16 == 4
