"""GPU: mvn_generate_windowed against the whole-context entry points, bit for bit, on every generator
variant with a conditioned form.  A launch over [t_begin, t_end) is handed a window that holds exactly those columns,
cut out of the whole time-major context and placed inside an allocation whose remainder is NaN: a kernel that read a
context word outside its stated set would carry the NaN into its logits, and the comparison with the ``context_tm`` run
(same launches, same state) would fail -- the read set is checked without touching unallocated memory."""
import functools

import numpy as np
import pytest
import torch

from helpers import DEV, synthetic_indices
from movenet_amd import _native as N
from movenet_amd.generation import RingGenerator, _stream_ptr
from movenet_amd.utils.weights import make_state_dict

pytestmark = pytest.mark.gpu

CFG2 = dict(layer_size=10, stack_size=3, input_channels=256, residual_channels=64, skip_channels=64)
CFG5 = dict(layer_size=10, stack_size=6, input_channels=256, residual_channels=128, skip_channels=128)
VARIANTS = {"GENERIC": (N.GEN_GENERIC, CFG2), "STREAM": (N.GEN_STREAM, CFG2), "PIPE": (N.GEN_PIPE, CFG2),
            "FOLD": (N.GEN_FOLD, CFG2), "PIPE_F16": (N.GEN_PIPE_F16, CFG5)}
N_NEW = 150
LAUNCHES = (1, 7, 64, 150)
SAMPLED = dict(sampling="model", temperature=1.0, top_k=32, top_p=0.9, seed=20261021)
PAD = 4096  # NaN words in front of and behind a window


@functools.lru_cache(maxsize=None)
def _weights(name):
    cfg = VARIANTS[name][1]
    return {k: v.to(DEV) for k, v in make_state_dict(**cfg, seed=1, gain=2.0, head_gain=6.0).items()}


def _generator(name, B, mode, guided=False):
    variant, cfg = VARIANTS[name]
    C = cfg["residual_channels"]
    dims = N.make_dims(**cfg)
    rf = N.lib().mvn_receptive_fields(dims)
    n_total = rf + N_NEW
    ctx = torch.from_numpy(np.random.default_rng(9).standard_normal((B, C, n_total)).astype(np.float32)).to(DEV)
    kw = dict(temperature=0.0) if mode == "greedy" else dict(SAMPLED)
    if guided:
        vec = torch.from_numpy(np.random.default_rng(4).standard_normal((B, C)).astype(np.float32)).to(DEV)
        kw.update(global_context=vec, guidance=[1.5, 0.5, 3.0][:B])
    g = RingGenerator(**cfg, state_dict=_weights(name), batch=B, n_total=n_total, device=DEV, variant=variant,
                      context=ctx, **kw)
    assert g.variant == variant
    g.prime(synthetic_indices(B, rf, cfg["input_channels"], 5).to(DEV))
    torch.cuda.synchronize()
    return g, rf, n_total


def _window(g, t0, t1):
    """Columns [t0, t1) of the generator's time-major context in the middle of a NaN-filled allocation."""
    C = g.dims.residual_channels
    n = t1 - t0
    raw = torch.full((2 * PAD + g.nrows * n * C,), float("nan"), device=DEV)
    win = raw[PAD:PAD + g.nrows * n * C].view(g.nrows, n, C)
    win.copy_(g.context_tm[:, t0:t1, :])
    return raw, win


def _launch_windowed(g, t0, t1, logits, choices, logits_t0):
    raw, win = _window(g, t0, t1)
    guided, scalar = g._guidance is not None, g._per_seq is None
    with torch.cuda.device(g.device):
        N.check(g.lib.mvn_generate_windowed(
            g.dims, g.variant, g.packed.data_ptr(), g.state.data_ptr(), g.samples_all.data_ptr(), g.batch,
            g.samples_all.stride(0), g.n_total, g.n_given, t0, t1, g.temperature if scalar else 0.0,
            g.seed if scalar else 0, g.top_k if scalar else 0, g.top_p if scalar else 1.0,
            None if scalar else g._per_seq.data_ptr(), g._guidance.data_ptr() if guided else None, logits.data_ptr(),
            choices.data_ptr(), logits_t0, win.data_ptr(), t0, t1 - t0, g._sampling, _stream_ptr(g.device)),
            "mvn_generate_windowed")
    return raw  # (kept alive until the run has been synchronised)


def _run(g, rf, n_total, step, windowed, primed):
    """N_NEW steps from the primed state in launches of ``step``: (samples, choices, logits) of all rows."""
    state0, samples0 = primed
    g.state.copy_(state0)
    g.samples_all.copy_(samples0)
    logits = torch.zeros(g.nrows, n_total - rf, g.Q, device=DEV)
    choices = torch.full((g.nrows, n_total), -1, dtype=torch.int32, device=DEV)
    keep = []
    t, t_end = rf - 1, rf - 1 + N_NEW
    while t < t_end:
        t1 = min(t + step, t_end)
        if windowed:
            keep.append(_launch_windowed(g, t, t1, logits, choices, rf))
        else:
            g._run(t, t1, g.n_given, logits, choices, rf)
        t = t1
    g.check_errors()  # (synchronises; a hand-off timeout would void the run)
    return g.samples_all.clone(), choices, logits


def _compare(name, B, mode, guided=False):
    g, rf, n_total = _generator(name, B, mode, guided)
    primed = (g.state.clone(), g.samples_all.clone())
    for step in LAUNCHES:
        want = _run(g, rf, n_total, step, False, primed)
        got = _run(g, rf, n_total, step, True, primed)
        for what, a, b in zip(("samples", "choices_out", "logits_out"), got, want):
            assert torch.equal(a, b), (name, mode, step, what)
        assert not bool(torch.isnan(got[2]).any()), (name, mode, step)
        assert bool((got[0][:, rf:] >= 0).all())
    if mode == "sampled":  # (the draws keep the clip moving: the comparison is not one class repeated)
        assert len(torch.unique(want[0][:, rf:])) > 8
    return want


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
@pytest.mark.parametrize("name", list(VARIANTS))
def test_windowed_launches_equal_whole_context_launches(name, mode):
    _compare(name, 2, mode)


@pytest.mark.parametrize("name", ["FOLD", "GENERIC"])
def test_guided_windowed_launches_equal_whole_context_launches(name):
    want = _compare(name, 3, "sampled", guided=True)
    samples = want[0]
    assert torch.equal(samples[:3, -N_NEW:], samples[3:, -N_NEW:])  # both rows of a pair carry the pair's picks


def test_a_window_one_column_short_is_refused_on_the_device_too():
    g, rf, n_total = _generator("GENERIC", 2, "greedy")
    before = (g.state.clone(), g.samples_all.clone())
    logits = torch.zeros(2, n_total - rf, g.Q, device=DEV)
    choices = torch.full((2, n_total), -1, dtype=torch.int32, device=DEV)
    raw, win = _window(g, rf, rf + 6)  # the launch reads column rf - 1 first
    with torch.cuda.device(DEV):
        rc = g.lib.mvn_generate_windowed(g.dims, g.variant, g.packed.data_ptr(), g.state.data_ptr(),
                                         g.samples_all.data_ptr(), 2, n_total, n_total, g.n_given, rf - 1, rf + 6, 0.0, 0,
                                         0, 1.0, None, None, logits.data_ptr(), choices.data_ptr(), rf, win.data_ptr(),
                                         rf, 6, g._sampling, _stream_ptr(g.device))
    assert rc == N.MVN_ERR_BAD_ARG and f"columns [{rf - 1}, {rf + 6})" in N.last_error()
    torch.cuda.synchronize()
    assert torch.equal(g.state, before[0]) and torch.equal(g.samples_all, before[1])
    assert bool((choices == -1).all()) and bool((logits == 0).all())
