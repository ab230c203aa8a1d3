"""CPU: global conditioning on a class label -- what needs no GPU: the module's parameters and RNG draws,
the trainer's class map, the ``--use_global`` flag and the new C-ABI symbols."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from movenet_amd import _native as N
from movenet_amd.config import TrainingConfig, arg_parser, config_from_args
from movenet_amd.wavenet import WaveNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mvn_context_add_global", "mvn_global_fast_path", "mvn_global_bias", "mvn_forward_global",
               "mvn_backward_global", "mvn_backward_scratch", "mvn_global_scratch_floats", "mvn_global_bias_backward")


def _seeded(**kw):
    torch.manual_seed(1234)
    return WaveNet(2, 2, 64, 16, 16, **kw).state_dict()


def test_zero_classes_is_the_module_as_it_was():
    plain, zero = _seeded(), _seeded(global_classes=0)
    assert list(plain) == list(zero)
    assert "global_embedding.weight" not in plain
    for k in plain:
        assert torch.equal(plain[k], zero[k]), k
    with pytest.raises(ValueError):
        WaveNet(2, 2, 64, 16, 16, global_classes=-1)


def test_classes_add_one_parameter_behind_all_others():
    plain, three = _seeded(), _seeded(global_classes=3)
    assert list(three) == list(plain) + ["global_embedding.weight"]
    assert three["global_embedding.weight"].shape == (3, 16)
    for k in plain:
        assert torch.equal(plain[k], three[k]), k
    m = WaveNet(2, 2, 64, 16, 16, global_classes=3)
    assert list(dict(m.named_parameters()))[-1] == "global_embedding.weight"
    assert m.global_path == "auto"
    assert not any(k.startswith("global_embedding") for k in m._decoder_state())


def test_global_vector_checks_need_no_device():
    from movenet_amd.ops import global_vector
    m = WaveNet(2, 2, 64, 16, 16, global_classes=3)
    E = m.global_embedding.weight
    assert global_vector(WaveNet(2, 2, 64, 16, 16), torch.tensor([5, 5]), 2) is None  # no classes: ignored
    assert torch.equal(global_vector(m, torch.tensor([2, 0]), 2), E[[2, 0]])
    rows = torch.tensor([[0.25, 0.75, 0.0], [0.0, 0.0, 1.0]])
    assert torch.allclose(global_vector(m, rows, 2), rows @ E)
    for bad in (None, torch.tensor([0]), torch.tensor([0, 3]), torch.tensor([-1, 0]), torch.rand(2, 4), torch.rand(3, 3),
                torch.tensor([0.0, 1.0])):
        with pytest.raises(ValueError):
            global_vector(m, bad, 2)


def test_class_map_from_the_training_contexts(tmp_path):
    import wav_material as WM
    from movenet_amd.pytorch_lightning_trainer import Dance2Music
    clips = WM.write_tree(tmp_path)
    contexts = sorted({c["context"] for c in clips})
    assert len(contexts) >= 2
    args = arg_parser().parse_args(["--dataset", str(tmp_path), "--use_video", "0", "--use_global", "1",
                                    "--input_channels", "64", "--layer_size", "2", "--stack_size", "2"])
    module = Dance2Music(str(tmp_path), config_from_args(args))
    assert module.global_classes == contexts
    assert module.model.global_classes == len(contexts)
    assert module.model.global_embedding.weight.shape[0] == len(contexts)
    got = module.class_indices([contexts[-1], contexts[0], contexts[-1]])
    assert got.tolist() == [len(contexts) - 1, 0, len(contexts) - 1] and got.dtype == torch.int64
    with pytest.raises(ValueError, match="waltz-of-nowhere"):
        module.class_indices([contexts[0], "waltz-of-nowhere"])
    # without the flag: no classes, no embedding, no labels
    args = arg_parser().parse_args(["--dataset", str(tmp_path), "--use_video", "0", "--input_channels", "64",
                                    "--layer_size", "2", "--stack_size", "2"])
    plain = Dance2Music(str(tmp_path), config_from_args(args))
    assert plain.global_classes == [] and plain.class_indices(contexts) is None
    assert "global_embedding.weight" not in plain.model.state_dict()
    # synthetic sources report one context
    synth = Dance2Music("synthetic://clips=2,frames=100", config_from_args(arg_parser().parse_args(
        ["--dataset", "synthetic://clips=2,frames=100", "--use_video", "0", "--use_global", "1"])))
    assert synth.global_classes == ["synthetic"] and synth.model.global_classes == 1


def test_use_global_flag():
    p = arg_parser()
    assert p.parse_args([]).use_global is False
    assert p.parse_args(["--use_global", "1"]).use_global is True
    assert config_from_args(p.parse_args(["--use_global", "1", "--use_video", "0"])).use_global is True
    assert TrainingConfig().use_global is False
    today = TrainingConfig().to_dict()
    assert today.pop("use_global") is False
    assert TrainingConfig.from_json(__import__("json").dumps(today)) == TrainingConfig()  # (a JSON written before the field)


def test_new_symbols_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "movenet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mvn_[a-z0-9_]+)\s*\(", text))
    lib = N.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in N.SIGNATURES, name
        assert hasattr(lib, name), name
    assert "#define MVN_BWD_FORM_ONE_GLOBAL 5" in open(os.path.join(ROOT, "include", "movenet_hip.h")).read()
    assert N.BWD_FORM_ONE_GLOBAL == 5 and N.BWD_FORM_ONE == 3
    # argument checks that need no device
    d = N.make_dims(3, 2, 64, 64, 64)
    assert lib.mvn_context_add_global(None, None, 1, 64, 10, 0, None) == N.MVN_ERR_BAD_ARG
    assert lib.mvn_global_bias(d, None, None, 1, None, None) == N.MVN_ERR_BAD_ARG
    assert lib.mvn_global_bias(N.make_dims(2, 2, 64, 16, 16), None, None, 1, None, None) == N.MVN_ERR_UNSUPPORTED
    assert lib.mvn_global_fast_path(N.make_dims(2, 2, 64, 16, 16), 2, 100) == 0
