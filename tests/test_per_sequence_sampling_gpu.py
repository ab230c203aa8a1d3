"""GPU: temperature, top_k, top_p and seed per sequence of a launch (mvn_generate_seq, include/movenet_hip.h) on all
five generator kernels, on the shapes and weights of tests/test_model_sampling_gpu.py, one kernel per shape as in
tests/test_truncated_sampling_gpu.py.  The contract under test: sequence b's step predicting time u does exactly what
mvn_generate_trunc does with per_seq[b]'s four values, on philox_uniform(per_seq[b].seed, u, per_seq[b].row)."""
import numpy as np
import pytest
import torch

import sampling_reference as R
import test_model_sampling_gpu as M
import test_truncated_sampling_gpu as T
from helpers import one_hot, synthetic_indices
from movenet_amd import _native as N
from movenet_amd.utils.weights import make_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES, RF, VARIANTS, ONE_PER_VARIANT = M.SHAPES, M.RF, M.VARIANTS, T.ONE_PER_VARIANT
IDS = [v for v, _ in ONE_PER_VARIANT]
PIPELINED = ("PIPE", "FOLD", "PIPE_F16")
# (temperature, top_k, top_p, seed): greedy, T = 0.5 and 1.0, k = 8, p = 0.9, both together, distinct seeds
TABLE = [(0.0, 0, 1.0, 11), (1.0, 0, 1.0, 12), (0.5, 8, 1.0, 13), (1.0, 0, 0.9, 14), (0.5, 8, 0.9, 15),
         (1.0, 8, 0.9, 16)]


def _gen(shape, batch, n_total, variant, settings=None, rows=None, **scalars):
    """RingGenerator under the model rule: ``settings`` a list of (T, k, p, seed), one per sequence, or scalars."""
    from movenet_amd.generation import RingGenerator
    if settings is not None:
        t, k, p, s = (list(c) for c in zip(*settings))
        scalars = dict(temperature=t, top_k=k, top_p=p, seed=s, rows=rows)
    g = RingGenerator(**SHAPES[shape], state_dict=M._weights(shape), batch=batch, n_total=n_total, device=DEV,
                      variant=VARIANTS[variant], sampling="model", **scalars)
    assert g.rf == RF[shape]
    assert (g._per_seq is not None) == (settings is not None)
    return g


def _table(B):
    return [TABLE[b % len(TABLE)] for b in range(B)]


def _hist(shape, B, n_new, seed=4321):
    return synthetic_indices(B, RF[shape] + n_new, SHAPES[shape]["input_channels"], seed).to(DEV)


def _pipes(variant, shape):
    pipes = N.lib().mvn_gen_launch_pipelines(N.make_dims(**SHAPES[shape]), VARIANTS[variant], 1 << 20)
    assert pipes >= 1
    return pipes


# ---- 1. rows equal scalar runs ---------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", ONE_PER_VARIANT, ids=IDS)
def test_each_row_equals_the_scalar_run_with_its_settings(variant, shape):
    """Teacher-forced, 48 steps.  Batches: 2, and for a pipelined kernel one sequence more than the launch has
    pipelines -- a pipeline of that launch's nb then serves sequences b and b + nb in turn, whose settings differ (nb
    is checked not to be a multiple of the table's length): where the settings followed the pipeline, one of the two
    would draw by the other's."""
    n_new, rf = 48, RF[shape]
    batches = [2] + ([_pipes(variant, shape) + 1] if variant in PIPELINED else [])
    for B in batches:
        settings, hist = _table(B), _hist(shape, B, n_new)
        if B > 2:
            nb = N.lib().mvn_gen_launch_pipelines(N.make_dims(**SHAPES[shape]), VARIANTS[variant], B)
            assert 1 <= nb < B and nb % len(TABLE) != 0 and settings[0] != settings[nb]
        g = _gen(shape, B, rf + n_new, variant, settings)
        choices, logits = g.teacher_forced(hist, logits_t0=rf)
        g.check_errors()
        choices, bits = choices[:, rf:].cpu().numpy(), logits.cpu().numpy().view(np.uint32)
        for (t, k, p, s) in sorted(set(settings)):
            gs = _gen(shape, B, rf + n_new, variant, temperature=t, top_k=k, top_p=p, seed=s)
            want, want_logits = gs.teacher_forced(hist, logits_t0=rf)
            gs.check_errors()
            want = want[:, rf:].cpu().numpy()
            assert np.array_equal(want_logits.cpu().numpy().view(np.uint32), bits)
            rows = [b for b in range(B) if settings[b] == (t, k, p, s)]
            for b in rows:
                assert np.array_equal(choices[b], want[b]), f"{variant} B={B} row {b} settings {(t, k, p, s)}"
        sampled = [b for b in range(B) if settings[b][0] > 0]
        assert all(len(np.unique(choices[b])) > 1 for b in sampled)


# ---- 2. all rows equal: mvn_generate_trunc to the bit ------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", ONE_PER_VARIANT, ids=IDS)
def test_equal_rows_reproduce_generate_trunc(variant, shape):
    rf, B, n_new, (t, k, p, s) = RF[shape], 4, 40, (1.0, 8, 0.9, 77)
    hist = _hist(shape, B, n_new)
    out = []
    for settings in (None, [(t, k, p, s)] * B):
        kw = dict(temperature=t, top_k=k, top_p=p, seed=s) if settings is None else {}
        g = _gen(shape, B, rf + n_new, variant, settings, **kw)
        choices, logits = g.teacher_forced(hist, logits_t0=rf)
        g.check_errors()
        g.prime(hist[:, :rf])
        g.advance(n_new)
        g.check_errors()
        out.append((choices.cpu().numpy(), logits.cpu().numpy().view(np.uint32), g.samples.cpu().numpy()))
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    assert len(np.unique(out[0][2][:, rf:])) > 1


# ---- 3. partition -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", ONE_PER_VARIANT, ids=IDS)
def test_a_free_run_split_at_an_odd_step_equals_one_call(variant, shape):
    rf, B, n_new = RF[shape], 6, 40
    prompt = _hist(shape, B, 0, seed=99)
    runs = []
    for parts in ((n_new,), (13, n_new - 13)):
        g = _gen(shape, B, rf + n_new, variant, _table(B))
        g.prime(prompt)
        for n in parts:
            g.advance(n)
        g.check_errors()
        runs.append(g.samples.clone())
    assert torch.equal(runs[0], runs[1])
    assert len(torch.unique(runs[0][:, rf:])) > 1


# ---- 4. position and plan -----------------------------------------------------------------------------------------
def _free_run(g, prompt, n_new):
    g.prime(prompt)
    g.advance(n_new)
    g.check_errors()
    return g.samples.clone()


@pytest.mark.parametrize("variant,shape", ONE_PER_VARIANT, ids=IDS)
def test_permuting_the_rows_permutes_the_output(variant, shape):
    rf, B, n_new = RF[shape], 6, 40
    prompt, settings = _hist(shape, B, 0, seed=99), _table(B)
    base = _free_run(_gen(shape, B, rf + n_new, variant, settings), prompt, n_new)
    perm = [4, 2, 0, 5, 1, 3]
    moved = _free_run(_gen(shape, B, rf + n_new, variant, [settings[i] for i in perm], rows=perm), prompt[perm], n_new)
    assert torch.equal(moved, base[perm])
    assert not torch.equal(base[1, rf:], base[2, rf:])


def test_grouped_equals_the_single_launch():
    from movenet_amd.generation import GroupedGenerator
    shape, rf, B, n_new = "S64", RF["S64"], 5, 60
    prompt, settings = _hist(shape, B, 0, seed=99), _table(B)
    single = _free_run(_gen(shape, B, rf + n_new, "FOLD", settings), prompt, n_new)
    t, k, p, s = (list(c) for c in zip(*settings))
    gg = GroupedGenerator(**SHAPES[shape], state_dict=M._weights(shape), batch=B, n_total=rf + n_new, device=DEV,
                          group=2, variant=N.GEN_FOLD, sampling="model", temperature=t, top_k=k, top_p=p, seed=s)
    assert gg.bounds == [(0, 2), (2, 4), (4, 5)]
    assert [g.rows for g in gg.groups] == [[0, 1], [2, 3], [4]]
    assert torch.equal(_free_run(gg, prompt, n_new), single)
    assert len(torch.unique(single[:, rf:])) > 1


@pytest.mark.parametrize("variant,shape", ONE_PER_VARIANT, ids=IDS)
def test_identical_rows_give_identical_sequences_and_the_seed_alone_changes_them(variant, shape):
    rf, n_new = RF[shape], 40
    prompt = _hist(shape, 1, 0, seed=99).repeat(3, 1)
    settings = [(1.0, 8, 0.9, 5), (1.0, 8, 0.9, 5), (1.0, 8, 0.9, 6)]
    out = _free_run(_gen(shape, 3, rf + n_new, variant, settings, rows=[7, 7, 7]), prompt, n_new)
    assert torch.equal(out[0], out[1])
    assert not torch.equal(out[0], out[2])


# ---- 5. against float64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", ONE_PER_VARIANT, ids=IDS)
def test_a_mixed_batch_against_float64_row_by_row(variant, shape):
    """One batch whose rows are the five settings of tests/test_truncated_sampling_gpu.py (every top_k < Q on all
    four shapes), seeds 100 + b, rows 40 - b: each row's 300 draws go through that file's _check_truncated_draws with
    philox_uniform(seed_b, u, row_b), its caps kept as conditions (unclear steps <= 1 % by top-k's criterion, <= 10 %
    in all).  300 draws per row keep the ORACLE's logits alone under the caps -- shares of unclear steps per row
    (top-k / all) from the CPU oracle on this history, rows in SETTINGS order:
        S16   0 / 0   0 / 0   0 / 0.0133   0 / 0   0 / 0.0067
        S64   0 / 0   0 / 0   0 / 0.0467   0 / 0   0 / 0.0067
        S64q  0 / 0   0 / 0   0 / 0.0100   0 / 0   0 / 0.0033
        S128  0 / 0   0 / 0   0 / 0.0600   0 / 0   0 / 0.0100
    (30 unclear steps of 300 would reach the cap; the worst row has 18.)"""
    rf, Q, n_new = RF[shape], SHAPES[shape]["input_channels"], 300
    assert all(k < Q for _, k, _ in T.SETTINGS)
    B = len(T.SETTINGS)
    settings = [(t, k, p, 100 + b) for b, (t, k, p) in enumerate(T.SETTINGS)]
    rows = [40 - b for b in range(B)]
    g = _gen(shape, B, rf + n_new, variant, settings, rows=rows)
    choices, logits = g.teacher_forced(_hist(shape, B, n_new), logits_t0=rf)
    g.check_errors()
    picks, logits = choices[:, rf:].cpu().numpy(), logits.cpu().numpy()
    for b, (t, k, p, s) in enumerate(settings):
        uniform = R.philox_uniform(s, np.arange(rf, rf + n_new)[None, :], np.array([[rows[b]]]))
        T._check_truncated_draws(picks[b:b + 1], logits[b:b + 1], t, k, p, uniform, Q,
                                 f"{variant} {shape} row {b} T={t} k={k} p={p}")


# ---- 6. WaveNet.generate with a temperature list ----------------------------------------------------------------
def test_wavenet_generate_with_a_temperature_per_sequence():
    from movenet_amd.wavenet import WaveNet
    cfg, rf, n_new = SHAPES["S64"], RF["S64"], 100
    model = WaveNet(**cfg)
    model.load_state_dict(make_state_dict(**cfg, seed=3, gain=2.0, head_gain=6.0), strict=False)
    model.to(DEV)
    model.generate_sampling = "model"
    prompt = one_hot(synthetic_indices(1, rf, 256, 11), 256).to(DEV)
    greedy = model.generate(prompt, n_samples=rf + n_new, temperature=0.0)
    temps = [1.0, 0.0, 0.5]
    out = model.generate(prompt.repeat(3, 1, 1), n_samples=rf + n_new, temperature=temps)
    assert out.shape == (3, 256, rf + n_new) and torch.equal(out.sum(1), torch.ones(3, rf + n_new, device=DEV))
    assert torch.equal(out[1], greedy[0])
    assert not torch.equal(out[0], greedy[0]) and not torch.equal(out[2], out[0])
    # keys per sequence: the same key and temperature twice is the same sequence only where the rows agree too
    model.generate_seed = [3, 3, 4]
    again = model.generate(prompt.repeat(3, 1, 1), n_samples=rf + n_new, temperature=[1.0, 1.0, 1.0])
    assert torch.equal(again, model.generate(prompt.repeat(3, 1, 1), n_samples=rf + n_new, temperature=[1.0] * 3))
    assert not torch.equal(again[0], again[1]) and not torch.equal(again[1], again[2])
    model.generate_seed = None
    for bad in ([1.0, 0.5], [1.0] * 4, torch.ones(3, 1)):
        with pytest.raises(ValueError, match="temperature"):
            model.generate(prompt.repeat(3, 1, 1), n_samples=rf + n_new, temperature=bad)
    model.generate_seed = [1, 2]
    with pytest.raises(ValueError, match="seed has 2 entries"):
        model.generate(prompt.repeat(3, 1, 1), n_samples=rf + n_new, temperature=1.0)


# ---- 7. guard bands -------------------------------------------------------------------------------------------
def test_guard_bands_stay_intact(monkeypatch):
    """Every kernel, a mixed batch with one sequence more than the pipelines where there are any, under
    MOVENET_DEBUG_GUARD=1: check_errors() compares the bands behind the packed weights and the state."""
    monkeypatch.setenv("MOVENET_DEBUG_GUARD", "1")
    for variant, shape in ONE_PER_VARIANT:
        rf, n_new = RF[shape], 24
        B = _pipes(variant, shape) + 1 if variant in PIPELINED else 3
        g = _gen(shape, B, rf + n_new, variant, _table(B))
        assert g._guard is not None
        out = _free_run(g, _hist(shape, B, 0, seed=99), n_new)
        Q = SHAPES[shape]["input_channels"]
        assert int(out.min()) >= 0 and int(out.max()) < Q
