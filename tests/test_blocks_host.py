"""CPU: the block entry points (mvn_block_*, csrc/blocks.hip) are declared, exported and bound; their scratch sizing and
every refusal are host arithmetic -- refused before any launch, with fake non-NULL pointers where a pointer is needed --
and the five block modules keep raising on the CPU."""
import os
import re

import pytest
import torch

from movenet_amd import _native as N
from movenet_amd import modules as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK_NAMES = [
    "mvn_block_last_form", "mvn_block_conv_scratch_floats",
    "mvn_block_causal_forward", "mvn_block_causal_backward",
    "mvn_block_dilated_forward", "mvn_block_dilated_backward",
    "mvn_block_gated_scratch_floats", "mvn_block_gated_forward", "mvn_block_gated_backward",
    "mvn_block_dense_scratch_floats", "mvn_block_dense_forward", "mvn_block_dense_backward",
]
FAKE = 0x10000  # a non-NULL address no refused call may touch


def bt(length, ld=None, p=FAKE):
    return N.BlockTensor(p, length if ld is None else ld, length)


def gated_params(ctx=True):
    vals = [FAKE] * 12
    vals[1] = vals[3] = None  # the dilated convs of the reference's layer carry no bias
    if not ctx:
        vals[4:8] = [None] * 4
    return N.BlockGatedParams(*vals)


def refused(rc, code, word=None):
    assert rc == code, (rc, N.last_error())
    text = N.last_error()
    assert text, "a refusal sets mvn_last_error()"
    if word:
        assert word in text, text


def test_block_names_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "movenet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mvn_[a-z0-9_]+)\s*\(", text))
    lib = N.lib()
    for name in BLOCK_NAMES:
        assert name in declared, f"{name} is not declared in movenet_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in N.SIGNATURES, f"{name} is not bound in _native.SIGNATURES"
    assert sorted(n for n in declared if n.startswith("mvn_block_")) == sorted(BLOCK_NAMES)
    assert "#define MVN_BLOCK_FORM_GENERIC 1" in text and "#define MVN_BLOCK_FORM_FUSED64 2" in text
    assert (N.BLOCK_FORM_GENERIC, N.BLOCK_FORM_FUSED64) == (1, 2)
    assert lib.mvn_abi_version() == 2
    assert lib.mvn_block_last_form() in (0, 1, 2)


def test_scratch_sizes_are_monotone_and_never_zero():
    lib = N.lib()
    sizes = {
        "conv": lambda B, T: lib.mvn_block_conv_scratch_floats(256, 64, B, T),
        "gated fwd": lambda B, T: lib.mvn_block_gated_scratch_floats(24, 40, B, T, 4, 0, 0),
        "gated fwd 64": lambda B, T: lib.mvn_block_gated_scratch_floats(64, 64, B, T, 4, 1, 0),
        "gated bwd": lambda B, T: lib.mvn_block_gated_scratch_floats(64, 64, B, T, 4, 0, 1),
        "gated bwd ctx": lambda B, T: lib.mvn_block_gated_scratch_floats(64, 64, B, T, 4, 1, 1),
        "dense fwd": lambda B, T: lib.mvn_block_dense_scratch_floats(64, 256, B, T, 0),
        "dense bwd": lambda B, T: lib.mvn_block_dense_scratch_floats(64, 256, B, T, 1),
    }
    Ts = (5, 6, 64, 65, 512, 513, 516, 517, 5000, 16000)
    for name, f in sizes.items():
        for B in (1, 2, 3, 16):
            vals = [f(B, T) for T in Ts]
            assert all(v > 0 for v in vals), (name, B, vals)
            assert vals == sorted(vals), (name, B, vals)
        for T in Ts:
            vals = [f(B, T) for B in (1, 2, 3, 16, 17)]
            assert vals == sorted(vals), (name, T, vals)
    # a context adds rows to the filter / gate weight gradient
    assert sizes["gated bwd ctx"](2, 600) >= sizes["gated bwd"](2, 600)
    # shapes the calls refuse size to 0
    assert lib.mvn_block_gated_scratch_floats(64, 64, 1, 4, 4, 0, 1) == 0      # T <= d
    assert lib.mvn_block_gated_scratch_floats(257, 64, 1, 40, 4, 0, 1) == 0
    assert lib.mvn_block_dense_scratch_floats(64, 1025, 1, 40, 1) == 0
    assert lib.mvn_block_conv_scratch_floats(0, 8, 1, 40) == 0


def test_conv_refusals():
    lib = N.lib()
    x, y = bt(40), bt(40)
    refused(lib.mvn_block_causal_forward(None, None, 16, 8, x, y, 1, None), N.MVN_ERR_BAD_ARG, "NULL")
    refused(lib.mvn_block_causal_forward(FAKE, None, 16, 8, None, y, 1, None), N.MVN_ERR_BAD_ARG, "x")
    refused(lib.mvn_block_causal_forward(FAKE, None, 16, 8, x, bt(40, p=None), 1, None), N.MVN_ERR_BAD_ARG, "y")
    refused(lib.mvn_block_causal_forward(FAKE, None, 16, 8, bt(40, ld=39), y, 1, None), N.MVN_ERR_BAD_ARG, "stride")
    refused(lib.mvn_block_causal_forward(FAKE, None, 16, 8, x, bt(39), 1, None), N.MVN_ERR_BAD_ARG, "length")
    refused(lib.mvn_block_causal_forward(FAKE, None, 16, 8, x, y, 0, None), N.MVN_ERR_BAD_ARG, "batch")
    refused(lib.mvn_block_causal_forward(FAKE, None, 1025, 8, x, y, 1, None), N.MVN_ERR_BAD_DIMS)
    big = bt(1 << 29)
    refused(lib.mvn_block_causal_forward(FAKE, None, 16, 8, big, big, 1, None), N.MVN_ERR_UNSUPPORTED, "2^31")
    need = lib.mvn_block_conv_scratch_floats(16, 8, 1, 40)
    refused(lib.mvn_block_causal_backward(FAKE, 16, 8, x, y, None, FAKE, None, 1, FAKE, need - 1, None),
            N.MVN_ERR_BAD_ARG, "scratch")
    refused(lib.mvn_block_causal_backward(FAKE, 16, 8, x, y, None, FAKE, None, 1, None, need, None),
            N.MVN_ERR_BAD_ARG, "scratch")
    # dilated: T <= d names both
    refused(lib.mvn_block_dilated_forward(FAKE, None, 8, 40, x, bt(1), 1, None), N.MVN_ERR_BAD_ARG, "T = 40")
    assert "d = 40" in N.last_error()
    refused(lib.mvn_block_dilated_forward(FAKE, None, 8, 4, x, bt(37), 1, None), N.MVN_ERR_BAD_ARG, "length")
    refused(lib.mvn_block_dilated_forward(FAKE, None, 257, 4, x, bt(36), 1, None), N.MVN_ERR_BAD_DIMS)
    refused(lib.mvn_block_dilated_backward(FAKE, 8, 4, x, bt(36), bt(39), FAKE, None, 1, FAKE, 1 << 30, None),
            N.MVN_ERR_BAD_ARG, "dx")
    refused(lib.mvn_block_dilated_backward(FAKE, 8, 4, x, bt(36), None, FAKE, None, 1, FAKE, 3, None),
            N.MVN_ERR_BAD_ARG, "scratch")


def test_gated_refusals():
    lib = N.lib()
    p, g = gated_params(), gated_params()
    T, d = 40, 4
    n = T - d
    x, res, skip, th, sg = bt(T), bt(n), bt(7), bt(n), bt(n)
    huge = 1 << 40

    def fwd(p=p, C=64, K=64, d=d, x=x, ctx=None, res=res, skip=skip, th=th, sg=sg, B=2, scratch=FAKE, ns=huge):
        return lib.mvn_block_gated_forward(p, C, K, d, x, ctx, res, skip, th, sg, B, scratch, ns, None)

    refused(fwd(p=None), N.MVN_ERR_BAD_ARG, "NULL")
    refused(fwd(x=None), N.MVN_ERR_BAD_ARG, "x")
    refused(fwd(res=None), N.MVN_ERR_BAD_ARG, "residual")
    refused(fwd(skip=None), N.MVN_ERR_BAD_ARG, "skip")
    refused(fwd(x=bt(T, ld=T - 1)), N.MVN_ERR_BAD_ARG, "stride")
    refused(fwd(d=T), N.MVN_ERR_BAD_ARG, f"T = {T}")
    refused(fwd(ctx=bt(n - 1)), N.MVN_ERR_BAD_ARG, "context")
    refused(fwd(p=gated_params(ctx=False), ctx=bt(n)), N.MVN_ERR_BAD_ARG, "context")
    refused(fwd(skip=bt(n + 1)), N.MVN_ERR_BAD_ARG, "skip")
    refused(fwd(sg=None), N.MVN_ERR_BAD_ARG, "together")
    refused(fwd(C=257), N.MVN_ERR_BAD_DIMS)
    refused(fwd(K=0), N.MVN_ERR_BAD_DIMS)
    refused(fwd(x=bt(1 << 29)), N.MVN_ERR_UNSUPPORTED, "2^31")
    # the generic form without saved activations keeps them in the scratch
    need = lib.mvn_block_gated_scratch_floats(24, 40, 2, T, d, 0, 0)
    assert need >= 2 * 2 * 24 * n
    refused(fwd(C=24, K=40, th=None, sg=None, ns=2 * 2 * 24 * n - 1), N.MVN_ERR_BAD_ARG, "scratch")
    refused(fwd(C=24, K=40, th=None, sg=None, scratch=None), N.MVN_ERR_BAD_ARG, "scratch")

    def bwd(p=p, g=g, C=64, K=64, d=d, x=x, ctx=None, th=th, sg=sg, dres=res, dskip=skip, dx=bt(T), dctx=None, B=2,
            scratch=FAKE, ns=huge):
        return lib.mvn_block_gated_backward(p, g, C, K, d, x, ctx, th, sg, dres, dskip, dx, dctx, B, scratch, ns, None)

    refused(bwd(g=None), N.MVN_ERR_BAD_ARG, "grads")
    refused(bwd(th=None), N.MVN_ERR_BAD_ARG, "th")
    refused(bwd(dres=None, dskip=None), N.MVN_ERR_BAD_ARG, "both NULL")
    refused(bwd(dx=bt(T - 1)), N.MVN_ERR_BAD_ARG, "dx")
    refused(bwd(dctx=bt(n)), N.MVN_ERR_BAD_ARG, "dcontext")
    refused(bwd(ctx=bt(n + 3), dctx=bt(n)), N.MVN_ERR_BAD_ARG, "dcontext")
    refused(bwd(ctx=bt(n - 1)), N.MVN_ERR_BAD_ARG, "context")
    refused(bwd(d=T + 1), N.MVN_ERR_BAD_ARG, f"d = {T + 1}")
    refused(bwd(C=300), N.MVN_ERR_BAD_DIMS)
    need = lib.mvn_block_gated_scratch_floats(64, 64, 2, T, d, 0, 1)
    refused(bwd(ns=need - 1), N.MVN_ERR_BAD_ARG, "scratch")
    refused(bwd(scratch=None, ns=need), N.MVN_ERR_BAD_ARG, "scratch")


def test_dense_refusals():
    lib = N.lib()
    x, h, y = bt(65), bt(65), bt(65)
    huge = 1 << 40
    refused(lib.mvn_block_dense_forward(FAKE, FAKE, FAKE, None, 64, 256, x, h, y, 1, None, 0, None), N.MVN_ERR_BAD_ARG, "NULL")
    refused(lib.mvn_block_dense_forward(FAKE, FAKE, FAKE, FAKE, 64, 256, x, h, bt(64), 1, None, 0, None),
            N.MVN_ERR_BAD_ARG, "length")
    refused(lib.mvn_block_dense_forward(FAKE, FAKE, FAKE, FAKE, 64, 256, x, None, y, 1, FAKE, 256 * 65 - 1, None),
            N.MVN_ERR_BAD_ARG, "scratch")
    refused(lib.mvn_block_dense_forward(FAKE, FAKE, FAKE, FAKE, 64, 1025, x, h, y, 1, None, 0, None), N.MVN_ERR_BAD_DIMS)
    refused(lib.mvn_block_dense_forward(FAKE, FAKE, FAKE, FAKE, 257, 256, x, h, y, 1, None, 0, None), N.MVN_ERR_BAD_DIMS)
    refused(lib.mvn_block_dense_forward(FAKE, FAKE, FAKE, FAKE, 64, 256, bt(1 << 29), h, y, 1, None, 0, None),
            N.MVN_ERR_UNSUPPORTED, "2^31")
    need = lib.mvn_block_dense_scratch_floats(64, 256, 1, 65, 1)
    refused(lib.mvn_block_dense_backward(FAKE, FAKE, 64, 256, x, h, y, None, FAKE, FAKE, FAKE, FAKE, 1, FAKE, need - 1, None),
            N.MVN_ERR_BAD_ARG, "scratch")
    refused(lib.mvn_block_dense_backward(FAKE, FAKE, 64, 256, x, None, y, None, FAKE, FAKE, FAKE, FAKE, 1, FAKE, huge, None),
            N.MVN_ERR_BAD_ARG, "hidden")
    refused(lib.mvn_block_dense_backward(FAKE, FAKE, 64, 256, x, h, bt(65, ld=64), None, FAKE, FAKE, FAKE, FAKE, 1, FAKE, huge,
                                         None), N.MVN_ERR_BAD_ARG, "dy")


def test_blocks_keep_raising_on_the_cpu():
    calls = [
        (M.CausalConv1d(16, 8), (torch.zeros(1, 16, 5),)),
        (M.DilatedCausalConv1d(8, dilation=2), (torch.zeros(1, 8, 5),)),
        (M.GatedResidualConv1d(8, 4, 2), (torch.zeros(1, 8, 5), None, 2)),
        (M.ResidualConvStack(2, 1, 8, 4), (torch.zeros(1, 8, 9), None, 2)),
        (M.DenseConv(4, 32), (torch.zeros(1, 4, 3),)),
    ]
    for block, args in calls:
        with pytest.raises(RuntimeError, match="holds parameters") as e:
            block(*args)
        assert "GPU tensors" in str(e.value)
    with pytest.raises(NotImplementedError, match="kernel_size = 3"):
        M.CausalConv1d(16, 8, kernel_size=3)(torch.zeros(1, 16, 5))
    with pytest.raises(NotImplementedError, match="kernel_size = 3"):
        M.DilatedCausalConv1d(8, dilation=2, kernel_size=3)(torch.zeros(1, 8, 9))
