"""CPU: the whole surface of the generator's host-side query functions, replayed against values recorded from the
library as it was BEFORE generate.hip was rewritten to drive one table of variant descriptors (csrc/gen_common.h:
GenVariant): mvn_gen_variant (return value and, where it fails, the mvn_last_error() text), mvn_gen_launch_pipelines,
mvn_gen_state_floats, mvn_gen_status_offset and mvn_gen_weights_floats, equal everywhere, strings included.

The grid: layer_size 1..10 x stack_size 1..9 (stage counts cross 32 per XCD for every pipelined variant), C = K in
{16, 64, 128, 256} and one C != K, Q in {16, 64, 128, 256, 512, 1024}, one invalid dims; variant ids -1..6 (two unknown
ones); the batches at which a variant's pipelines, rounds and limits change.  With no device visible the library
assumes 256 CUs, the MI355X's count, so the values are the same with and without a GPU.

The fixture (tests/golden/gen_variant_table.npz: the arrays sweep() returns, plus the grid) was written once, from a
library built at the commit before the table; there is no mode that rewrites it -- recorded from the code under test
it would say nothing.
"""
import itertools
import os

import numpy as np

from movenet_amd import _native as N

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_variant_table.npz")

CHANNELS = ((16, 16), (64, 64), (128, 128), (256, 256), (64, 128))      # (C, K)
CLASSES = (16, 64, 128, 256, 512, 1024)
VARIANTS = tuple(range(-1, 7))
BATCHES = (0, 1, 16, 17, 64, 65, 80, 81, 184, 185, 192, 193, 512)


def grid():
    """(layer_size, stack_size, Q, C, K) rows; the last one is invalid (layer_size 0)."""
    rows = [(ls, ss, q, c, k) for ls, ss, (c, k), q in
            itertools.product(range(1, 11), range(1, 10), CHANNELS, CLASSES)]
    return np.array(rows + [(0, 3, 256, 64, 64)], dtype=np.int32)


def sweep(dims_rows):
    """Every query at every grid point.  Error texts are interned: `err` holds indices into `texts` (-1: the call
    succeeded)."""
    lib = N.lib()
    n, nv, nb = len(dims_rows), len(VARIANTS), len(BATCHES)
    rc = np.zeros((n, nv, nb), np.int32)
    pipes = np.zeros((n, nv, nb), np.int32)
    err = np.full((n, nv, nb), -1, np.int32)
    state = np.zeros((n, nb), np.uint64)
    status = np.zeros((n, nb), np.uint64)
    weights = np.zeros((n, nv), np.uint64)
    texts = {}
    gen_variant, launch_pipelines, last_error = lib.mvn_gen_variant, lib.mvn_gen_launch_pipelines, lib.mvn_last_error
    for i, row in enumerate(dims_rows):
        d = N.make_dims(*(int(v) for v in row))
        for j, v in enumerate(VARIANTS):
            for k, b in enumerate(BATCHES):
                r = rc[i, j, k] = gen_variant(d, v, b)
                if r < 0:
                    err[i, j, k] = texts.setdefault(last_error(), len(texts))
                pipes[i, j, k] = launch_pipelines(d, v, b)
            weights[i, j] = lib.mvn_gen_weights_floats(d, v)
        for k, b in enumerate(BATCHES):
            state[i, k] = lib.mvn_gen_state_floats(d, b)
            status[i, k] = lib.mvn_gen_status_offset(d, b)
    texts = np.array([t.decode() for t in sorted(texts, key=texts.get)])
    return dict(rc=rc, pipes=pipes, err=err, texts=texts, state=state, status=status, weights=weights)


def test_query_surface_equals_the_recording():
    fx = np.load(FIXTURE, allow_pickle=False)
    dims_rows = grid()
    assert np.array_equal(fx["dims"], dims_rows) and tuple(fx["variants"]) == VARIANTS and tuple(fx["batches"]) == BATCHES
    got = sweep(dims_rows)
    for key in ("rc", "pipes", "state", "status", "weights"):
        bad = np.argwhere(got[key] != fx[key])
        assert len(bad) == 0, f"{key}: {len(bad)} points differ, first at dims {dims_rows[bad[0][0]]} index {bad[0][1:]}: " \
                              f"{got[key][tuple(bad[0])]} != {fx[key][tuple(bad[0])]}"
    # the texts themselves, point by point (the interning order is the sweep's, so the indices agree too)
    assert np.array_equal(got["err"] >= 0, fx["err"] >= 0)
    want_text, got_text = fx["texts"][fx["err"]], got["texts"][got["err"]]
    bad = np.argwhere((got_text != want_text) & (fx["err"] >= 0))
    assert len(bad) == 0, f"error text: {len(bad)} points differ, first at dims {dims_rows[bad[0][0]]}: " \
                          f"{got_text[tuple(bad[0])]!r} != {want_text[tuple(bad[0])]!r}"
    # every family of outcome is in the grid: each variant accepted, refusals, unknown ids, bad dims
    assert {int(v) for v in np.unique(fx["rc"])} == {N.MVN_ERR_UNSUPPORTED, N.MVN_ERR_BAD_ARG, N.MVN_ERR_BAD_DIMS,
                                                    N.GEN_GENERIC, N.GEN_STREAM, N.GEN_PIPE, N.GEN_PIPE_F16, N.GEN_FOLD}

