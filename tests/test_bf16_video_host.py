"""No GPU: the surface of video-conditioned bf16 training -- the C symbols (mvn_forward_bf16_ctx, mvn_backward_bf16_ctx,
mvn_bf16_ctx_path, mvn_bf16_ctx_scratch_floats, MVN_BWD_FORM_BF16_CTX), the argument checks that need no device, the
truth table of ops.bf16_mode over (bf16_context, conditioned, labelled, global_path), the CLI flag and the Trainer's
argument check."""
import itertools
import re
from pathlib import Path

import pytest

from movenet_amd import _native as N
from movenet_amd import ops

ROOT = Path(__file__).resolve().parents[1]
SYMBOLS = ("mvn_forward_bf16_ctx", "mvn_backward_bf16_ctx", "mvn_bf16_ctx_path", "mvn_bf16_ctx_scratch_floats")


def test_symbols_declared_signed_and_exported():
    header = (ROOT / "include" / "movenet_hip.h").read_text()
    lib = N.lib()
    for name in SYMBOLS:
        assert re.search(r"\b(int|size_t) " + name + r"\(", header), name
        assert name in N.SIGNATURES, name
        assert hasattr(lib, name), name
    assert re.search(r"#define MVN_BWD_FORM_BF16_CTX 7\b", header)
    assert N.BWD_FORM_BF16_CTX == 7
    assert len(N.SIGNATURES["mvn_forward_bf16_ctx"][1]) == len(N.SIGNATURES["mvn_forward_bf16"][1])
    # (the backward takes mvn_backward_bf16's arguments and, in front of the stream, the scratch and its size)
    assert len(N.SIGNATURES["mvn_backward_bf16_ctx"][1]) == len(N.SIGNATURES["mvn_backward_bf16"][1]) + 2


def test_argument_checks_without_a_device():
    lib = N.lib()
    d64, d16 = N.make_dims(2, 2, 64, 64, 64), N.make_dims(2, 2, 64, 16, 16)
    B, T = 2, 300
    assert lib.mvn_bf16_ctx_path(d64, B, T) == 1
    assert lib.mvn_bf16_ctx_path(d16, B, T) == 0
    assert lib.mvn_bf16_ctx_path(d64, 0, T) == 0
    assert lib.mvn_bf16_ctx_path(d64, B, (1 << 21) + 64) == 0
    assert lib.mvn_bf16_ctx_scratch_floats(d64, B, T) >= 2 * B * 64 * lib.mvn_padded_len(T)
    assert lib.mvn_bf16_ctx_scratch_floats(d16, 0, T) == 0
    empty = N.FwdBuffers(None, None, None, None, None, None, None, 0, None, 0)
    # the dims are refused first (MVN_ERR_UNSUPPORTED), then a missing context (MVN_ERR_BAD_ARG): nothing is launched
    rc = lib.mvn_forward_bf16_ctx(d16, None, None, T, B, T, empty, None, 0, 1, 1, None)
    assert rc == N.MVN_ERR_UNSUPPORTED and "residual_channels = skip_channels = 64" in lib.mvn_last_error().decode()
    rc = lib.mvn_forward_bf16_ctx(d64, None, None, T, B, T, empty, None, 0, 1, 1, None)
    assert rc == N.MVN_ERR_BAD_ARG and "no context" in lib.mvn_last_error().decode()
    rc = lib.mvn_backward_bf16_ctx(d16, None, None, None, T, B, T, empty, None, None, None, 0, 1, None, 0, None)
    assert rc == N.MVN_ERR_UNSUPPORTED
    rc = lib.mvn_backward_bf16_ctx(d64, None, None, None, T, B, T, empty, None, None, None, 0, 1, None, 0, None)
    assert rc == N.MVN_ERR_BAD_ARG and "no context" in lib.mvn_last_error().decode()
    rc = lib.mvn_forward_bf16_ctx(d64, None, None, T, B, (1 << 21) + 64, empty, None, 0, 1, 1, None)
    assert rc == N.MVN_ERR_UNSUPPORTED and "t_len" in lib.mvn_last_error().decode()


class _Model:
    def __init__(self, precision, bf16_context, path, C=64):
        self.forward_precision, self.bf16_context, self.global_path = precision, bf16_context, path
        self._dims = N.make_dims(2, 2, 64, C, C)


def _today(conditioned, labelled, path):
    """bf16_mode as it was before the switch existed."""
    if conditioned:
        return "no video context"
    if labelled and path != "bias":
        return "no global conditioning"
    return True


@pytest.mark.parametrize("bf16_context,conditioned,labelled,path",
                         list(itertools.product((False, True), (False, True), (False, True), ("auto", "context", "bias"))))
def test_bf16_mode_truth_table(bf16_context, conditioned, labelled, path):
    m = _Model("bf16", bf16_context, path)
    if bf16_context and conditioned:
        want = "global_path 'bias' runs models without a video context" if (labelled and path == "bias") else True
    else:
        want = _today(conditioned, labelled, path)
    if want is True:
        assert ops.bf16_mode(m, conditioned, labelled) is True
    else:
        with pytest.raises(ValueError, match=want):
            ops.bf16_mode(m, conditioned, labelled)
    assert ops.bf16_mode(_Model("fp32", bf16_context, path), conditioned, labelled) is False
    with pytest.raises(ValueError, match="residual_channels = skip_channels = 64"):
        ops.bf16_mode(_Model("bf16", bf16_context, path, C=16), conditioned, labelled)


def test_model_switch_defaults_off():
    from movenet_amd.wavenet import WaveNet
    m = WaveNet(layer_size=2, stack_size=2, input_channels=64, residual_channels=64, skip_channels=64)
    assert m.bf16_context is False


def test_cli_flag_and_trainer_argument():
    from movenet_amd.config import arg_parser, config_from_args
    from movenet_amd.pytorch_lightning_trainer import Trainer
    base = ["--dataset", "synthetic://clips=2,frames=400"]
    assert config_from_args(arg_parser().parse_args(base)).bf16_video is False
    assert config_from_args(arg_parser().parse_args(base + ["--bf16_video", "1"])).bf16_video is True
    with pytest.raises(ValueError, match="bf16_video"):
        Trainer(max_epochs=1, precision=32, bf16_video=True)
    assert Trainer(max_epochs=1, precision="bf16", bf16_video=True).bf16_video is True
    assert Trainer(max_epochs=1, precision="bf16").bf16_video is False
