"""No GPU: the refusals of the full-sequence backward are all decided in front of its first launch (sequence.hip
plan_backward).  Every call here must refuse, so nothing is ever launched: the buffers are host structs whose device
pointers are dummy non-null values, and without a device the library plans for 256 CUs.  A refused call leaves
mvn_last_backward_form() and mvn_last_embed_form() as they were."""
import ctypes as C

import pytest

from movenet_amd import _native as N

DUMMY = 0x1000  # never dereferenced: every case returns before its first launch


def _ptrs(n):
    return C.cast((C.c_void_p * n)(*([DUMMY] * n)), N._PP)


def _buffers(L, ctx=False, z=True):
    per_layer = {k: _ptrs(L) for k in ("filter_w", "gate_w", "residual_w", "residual_b", "skip_w", "skip_b",
                                       "ctx_filter_w", "ctx_filter_b", "ctx_gate_w", "ctx_gate_b")}
    flat = {k: DUMMY for k in ("causal_w", "head1_w", "head1_b", "head2_w", "head2_b")}
    params, grads = N.Params(**per_layer, **flat), N.ParamGrads(**per_layer, **flat)
    fwd = N.FwdBuffers(DUMMY, DUMMY, DUMMY, DUMMY if z else None, DUMMY, DUMMY, DUMMY if ctx else None, 1 << 20, None, 0)
    bwd = N.BwdBuffers(DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY if ctx else None)
    return params, grads, fwd, bwd


def _rf(layer_size, stack_size):
    return stack_size * (2 ** layer_size - 1) + 1


def _refused(call, rc, text):
    lib = N.lib()
    form, embed = lib.mvn_last_backward_form(), lib.mvn_last_embed_form()
    got = call(lib)
    assert got == rc, (got, lib.mvn_last_error().decode())
    assert text in lib.mvn_last_error().decode(), lib.mvn_last_error().decode()
    assert lib.mvn_last_backward_form() == form
    assert lib.mvn_last_embed_form() == embed


def test_embed_form_constants_match_the_header():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "movenet_hip.h")).read()
    for name, value in (("DENSE", 1), ("MFMA", 2), ("LDS", 3), ("TABLES", 4), ("ATOMICS", 5)):
        assert re.search(rf"#define MVN_EMBED_FORM_{name} {value}\b", header), name
        assert getattr(N, "EMBED_FORM_" + name) == value
    assert 0 <= N.lib().mvn_last_embed_form() <= 5   # (0: no backward in this process yet)


def test_embedding_gradient_refusal_comes_before_every_launch():
    # input_channels > 8192 with an index: once the last statement of the backward, behind every launch
    d, B, T = N.make_dims(2, 1, 8200, 64, 64), 1, _rf(2, 1) + 8
    p, g, fwd, bwd = _buffers(2)
    _refused(lambda lib: lib.mvn_backward(d, p, g, DUMMY, T, B, T, fwd, bwd, DUMMY, DUMMY, 1, 1, None),
             N.MVN_ERR_UNSUPPORTED, "input_channels 8200 > 8192 not supported by the embedding gradient")


def test_bf16_slabs_fit_nowhere():
    # da1 = (2, 64, Sp) holds no workgroup's slabs per sequence, and there is no z scratch to take them instead
    d, B, T = N.make_dims(3, 1, 64, 64, 64), 2, _rf(3, 1) + 40
    p, g, fwd, bwd = _buffers(3, z=False)
    _refused(lambda lib: lib.mvn_backward_bf16(d, p, g, DUMMY, T, B, T, fwd, bwd, DUMMY, DUMMY, 1, 1, None),
             N.MVN_ERR_UNSUPPORTED, "slabs do not fit the scratch at batch 2")


def test_backward_global_refuses_a_context():
    d, B, T = N.make_dims(3, 1, 64, 64, 64), 2, _rf(3, 1) + 40
    p, g, fwd, bwd = _buffers(3, ctx=True)
    n = N.lib().mvn_global_scratch_floats(d, B, T)
    _refused(lambda lib: lib.mvn_backward_global(d, p, g, DUMMY, T, B, T, fwd, bwd, DUMMY, DUMMY, 1, 1, DUMMY, n, DUMMY,
                                                 None),
             N.MVN_ERR_UNSUPPORTED, "mvn_backward_global: needs the one-kernel layer backward")


def test_bf16_ctx_refuses_a_short_scratch():
    d, B, T = N.make_dims(3, 1, 64, 64, 64), 2, _rf(3, 1) + 40
    p, g, fwd, bwd = _buffers(3, ctx=True)
    n = N.lib().mvn_bf16_ctx_scratch_floats(d, B, T)
    assert n > 0
    _refused(lambda lib: lib.mvn_backward_bf16_ctx(d, p, g, DUMMY, T, B, T, fwd, bwd, DUMMY, DUMMY, 1, 1, DUMMY, n - 1,
                                                   None),
             N.MVN_ERR_BAD_ARG, "mvn_bf16_ctx_scratch_floats()")


@pytest.mark.parametrize("entry", ["mvn_backward", "mvn_backward_bf16"])
def test_refusals_keep_their_order(entry):
    # a NULL buffer is still refused in front of the size-dependent refusals that moved
    d, B, T = N.make_dims(2, 1, 8200, 64, 64), 1, _rf(2, 1) + 8
    p, g, fwd, bwd = _buffers(2)
    bwd.dlogit = None
    _refused(lambda lib: getattr(lib, entry)(d, p, g, DUMMY, T, B, T, fwd, bwd, DUMMY, DUMMY, 1, 1, None),
             N.MVN_ERR_BAD_ARG, "mvn_backward: NULL buffer")
