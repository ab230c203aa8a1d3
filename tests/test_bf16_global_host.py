"""CPU: labelled training in bf16 -- what needs no GPU: the four new C-ABI symbols and their
refusals, the ``global_path = "bias"`` setter, and the emulation the GPU tests calibrate against."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bf16_emulation as E
import bf16_global_emulation as EG
from helpers import one_hot, synthetic_indices
from movenet_amd import _native as N
from movenet_amd.utils.weights import make_state_dict
from movenet_amd.wavenet import WaveNet
from oracle import wavenet_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mvn_global_bf16_path", "mvn_global_bf16_scratch_floats", "mvn_forward_bf16_global",
               "mvn_backward_bf16_global")


def test_symbols_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "movenet_hip.h")).read()
    assert "#define MVN_BWD_FORM_BF16_GLOBAL 6" in text and N.BWD_FORM_BF16_GLOBAL == 6
    assert "#define MVN_ABI_VERSION 2" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mvn_[a-z0-9_]+)\s*\(", code))
    lib = N.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in N.SIGNATURES and hasattr(lib, name), name
    # the header's signatures: the audio-only / fp32 twins' arguments with the label's ones in the documented places
    assert N.SIGNATURES["mvn_global_bf16_path"] == N.SIGNATURES["mvn_global_fast_path"]
    assert N.SIGNATURES["mvn_global_bf16_scratch_floats"] == N.SIGNATURES["mvn_global_scratch_floats"]
    res, args = N.SIGNATURES["mvn_forward_bf16"]
    assert N.SIGNATURES["mvn_forward_bf16_global"] == (res, args[:-1] + [C.c_void_p, args[-1]])
    res, args = N.SIGNATURES["mvn_backward_bf16"]
    assert N.SIGNATURES["mvn_backward_bf16_global"] == (res, args[:-1] + [C.c_void_p, C.c_size_t, C.c_void_p, args[-1]])
    assert N.SIGNATURES["mvn_forward_bf16_global"] == N.SIGNATURES["mvn_forward_global"]
    assert N.SIGNATURES["mvn_backward_bf16_global"] == N.SIGNATURES["mvn_backward_global"]


def test_path_and_scratch_answers_need_no_device():
    lib = N.lib()
    d64, d16, mixed = N.make_dims(2, 2, 64, 64, 64), N.make_dims(2, 2, 64, 16, 16), N.make_dims(2, 2, 64, 64, 32)
    assert lib.mvn_global_bf16_path(d64, 2, 300) == 1
    assert lib.mvn_global_bf16_path(d16, 2, 300) == 0
    assert lib.mvn_global_bf16_path(mixed, 2, 300) == 0
    assert lib.mvn_global_bf16_path(d64, 0, 300) == 0
    assert lib.mvn_global_bf16_path(d64, 1, (1 << 21) + 1) == 0  # (rows past the bf16 layer kernels' limit)
    per_wg = 128 * 64 + 128 * 128 + 128 + 128  # a workgroup's two slabs, its bias partials, its row-sum partials
    n = int(lib.mvn_global_bf16_scratch_floats(d64, 2, 300))
    assert n > 0 and n % (2 * per_wg) == 0
    # never more workgroups than 64-step tiles of the longest layer (T = 300, d = 1: columns 0 .. 299, five tiles)
    assert n <= 5 * 2 * per_wg
    assert int(lib.mvn_global_bf16_scratch_floats(d64, 0, 300)) == 0


def test_refusals_need_no_device():
    lib = N.lib()
    d64, d16 = N.make_dims(2, 2, 64, 64, 64), N.make_dims(2, 2, 64, 16, 16)
    word = (C.c_float * 4)()
    live = C.addressof(word)  # (a refused call reads and writes nothing: any non-NULL address will do)
    ctx_buf = N.FwdBuffers(live, live, live, live, live, live, live, 320, None, 0)
    plain = N.FwdBuffers(live, live, live, live, live, live, None, 0, None, 0)
    need = int(lib.mvn_global_bf16_scratch_floats(d64, 2, 300))

    def fwd(dims, buf, gbias):
        return lib.mvn_forward_bf16_global(dims, None, None, 0, 2, 300, buf, None, 0, 1, 1, gbias, None)

    def bwd(dims, buf, scratch, n, rowsum):
        return lib.mvn_backward_bf16_global(dims, None, None, None, 0, 2, 300, buf, None, None, None, 0, 1, scratch, n,
                                            rowsum, None)

    assert fwd(d16, plain, live) == N.MVN_ERR_UNSUPPORTED and b"64" in lib.mvn_last_error()
    assert fwd(d64, ctx_buf, live) == N.MVN_ERR_UNSUPPORTED and b"context" in lib.mvn_last_error()
    assert fwd(d64, plain, None) == N.MVN_ERR_BAD_ARG and b"gbias" in lib.mvn_last_error()
    assert bwd(d16, plain, live, need, live) == N.MVN_ERR_UNSUPPORTED and b"64" in lib.mvn_last_error()
    assert bwd(d64, ctx_buf, live, need, live) == N.MVN_ERR_UNSUPPORTED and b"context" in lib.mvn_last_error()
    assert bwd(d64, plain, None, need, live) == N.MVN_ERR_BAD_ARG and b"NULL" in lib.mvn_last_error()
    assert bwd(d64, plain, live, need, None) == N.MVN_ERR_BAD_ARG and b"NULL" in lib.mvn_last_error()
    assert bwd(d64, plain, live, need - 1, live) == N.MVN_ERR_BAD_ARG
    assert b"mvn_global_bf16_scratch_floats" in lib.mvn_last_error()
    # the audio-only forward refuses a context as it did (mvn_backward_bf16 checks its buffers first: on the GPU)
    assert lib.mvn_forward_bf16(d64, None, None, 0, 2, 300, ctx_buf, None, 0, 1, 1, None) == N.MVN_ERR_UNSUPPORTED


def test_global_path_setter():
    m = WaveNet(2, 2, 64, 16, 16, global_classes=3)
    assert m.global_path == "auto"
    for value in ("bias", "context", "auto"):
        m.global_path = value
        assert m.global_path == value
    for bad in ("fast", "bf16", "", None):
        with pytest.raises(ValueError):
            m.global_path = bad
    assert m.global_path == "auto"


def test_bf16_mode_lets_labels_through_under_bias_only():
    from movenet_amd.ops import bf16_mode
    m = WaveNet(2, 2, 64, 64, 64, global_classes=3)
    m.forward_precision = "bf16"
    for path in ("auto", "context"):
        m.global_path = path
        with pytest.raises(ValueError, match="global"):
            bf16_mode(m, False, True)
    m.global_path = "bias"
    assert bf16_mode(m, False, True) is True
    with pytest.raises(ValueError, match="no video context"):
        bf16_mode(m, True, True)
    m16 = WaveNet(2, 2, 64, 16, 16, global_classes=3)
    m16.forward_precision, m16.global_path = "bf16", "bias"
    with pytest.raises(ValueError, match="residual_channels = skip_channels = 64"):
        bf16_mode(m16, False, True)


def test_emulation_without_a_label_is_the_audio_only_emulation():
    cfg = dict(layer_size=2, stack_size=2, input_channels=64, residual_channels=64, skip_channels=64)
    sd = dict(make_state_dict(**cfg, seed=5))
    for k in sd:
        if "context_conv" in k and k.endswith(".bias"):
            sd[k] = torch.zeros_like(sd[k])
    dims = O.Dims(**cfg)
    x = one_hot(synthetic_indices(2, 90, 64, 6), 64)
    with torch.no_grad():
        want = E.logits(sd, dims, x)
        got = EG.logits(sd, dims, x, torch.zeros(2, 64))
        moved = EG.logits(sd, dims, x, torch.ones(2, 64))
    assert torch.equal(got, want)
    assert not torch.equal(moved, want)  # (the term is there)
