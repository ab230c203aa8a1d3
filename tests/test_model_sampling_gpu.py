"""GPU: the "model" sampling rule of the generators (MVN_SAMPLE_MODEL, include/movenet_hip.h) -- a sampled step draws
from the model's own softmax(logits / T) instead of the reference's softmax(softmax(logits) / T).

Every draw of every kernel is checked against the float64 inverse CDF of the kernel's own logits and the exact Philox
uniform (tests/sampling_reference.py); the frequencies of one step against the CPU oracle's logits; and the rule must
change nothing but the choice of a sampled step.

Bounds.  eps = 2^-14 on a CDF edge: four times the worst rounding of a 256-term fp32 running sum (256 x 2^-24), which
also covers the 1-2 ulp of v_exp_f32 / v_rcp_f32.  Matching share >= 99.9 %: the project's figure for draws within
rounding of a CDF edge (test_generate_gpu.py).  Frequencies: 6 standard errors sqrt(p (1 - p) / n) per bin, classes with
n p < 16 pooled into one bin."""
import functools

import numpy as np
import pytest
import torch

import sampling_reference as R
from helpers import one_hot, synthetic_indices
from movenet_amd import _native as N
from movenet_amd.utils.weights import make_state_dict
from oracle import wavenet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -14
SEED = 77


def _cfg(layer_size, stack_size, Q, C, K):
    return dict(layer_size=layer_size, stack_size=stack_size, input_channels=Q, residual_channels=C, skip_channels=K)


SHAPES = {"S64": _cfg(4, 1, 256, 64, 64), "S64q": _cfg(4, 1, 64, 64, 64), "S128": _cfg(5, 2, 256, 128, 128),
          "S16": _cfg(2, 2, 64, 16, 16)}
RF = {"S64": 16, "S64q": 16, "S128": 64, "S16": 8}
VARIANTS = {"GENERIC": N.GEN_GENERIC, "STREAM": N.GEN_STREAM, "PIPE": N.GEN_PIPE, "FOLD": N.GEN_FOLD,
            "PIPE_F16": N.GEN_PIPE_F16}
# (variant, shape, B, n_new); S64q (a 64-class model on the 256-wide heads: 192 padded classes) wherever
# mvn_gen_variant takes it on a tuned kernel
CASES = [("GENERIC", "S16", 16, 700), ("GENERIC", "S64", 16, 700), ("STREAM", "S64", 16, 700),
         ("PIPE", "S64", 16, 700), ("FOLD", "S64", 16, 700), ("PIPE", "S64q", 16, 700), ("FOLD", "S64q", 16, 700),
         ("STREAM", "S64q", 16, 700), ("PIPE_F16", "S128", 8, 300)]
CASE_IDS = [f"{v}-{s}" for v, s, _, _ in CASES]


@functools.lru_cache(maxsize=None)
def _weights(shape):
    return {k: v.to(DEV) for k, v in make_state_dict(**SHAPES[shape], seed=3, gain=2.0, head_gain=6.0).items()}


def _gen(shape, batch, n_total, variant, temperature=0.0, seed=0, sampling="reference"):
    from movenet_amd.generation import RingGenerator
    g = RingGenerator(**SHAPES[shape], state_dict=_weights(shape), batch=batch, n_total=n_total, device=DEV,
                      variant=VARIANTS[variant] if isinstance(variant, str) else variant, temperature=temperature,
                      seed=seed, sampling=sampling)
    assert g.rf == RF[shape]
    return g


_MODEL_RUNS = {}  # the "model" runs at T = 1.0: computed once, used by tests 1 and 2


def _teacher_forced(variant, shape, B, n_new, T, sampling):
    """(picks (B, n_new) for times rf .. rf + n_new - 1, logits (B, n_new, Q)) of one teacher-forced run, as numpy."""
    key = (variant, shape, B, n_new)
    if sampling == "model" and T == 1.0 and key in _MODEL_RUNS:
        return _MODEL_RUNS[key]
    rf, Q = RF[shape], SHAPES[shape]["input_channels"]
    g = _gen(shape, B, rf + n_new, variant, temperature=T, seed=SEED, sampling=sampling)
    hist = synthetic_indices(B, rf + n_new, Q, 4321).to(DEV)
    choices, logits = g.teacher_forced(hist, logits_t0=g.rf)
    g.check_errors()
    out = choices[:, rf:].cpu().numpy(), logits.cpu().numpy()
    if sampling == "model" and T == 1.0:
        _MODEL_RUNS[key] = out
    return out


def _uniforms(seed, rf, B, n_new):
    """philox_uniform(seed, u, b) for u = rf .. rf + n_new - 1, b = 0 .. B - 1, as (B, n_new)."""
    return R.philox_uniform(seed, np.arange(rf, rf + n_new)[None, :], np.arange(B)[:, None])


def _check_draws(picks, logits, T, uniform, Q, what):
    """Conditions (a) - (c) on every draw."""
    assert logits.shape == picks.shape + (Q,) and np.isfinite(logits).all()
    assert picks.min() >= 0 and picks.max() < Q, f"{what}: picks outside [0, {Q})"                      # (a)
    cdf = R.model_cdf(logits, T)
    excess = R.band_excess(picks, cdf, uniform)
    same = (picks == R.inverse_cdf_picks(cdf, uniform)).mean()
    print(f"{what}: worst excess over the float64 band {excess.max():.3g} (eps {EPS:.3g}), picks equal to float64's "
          f"on {same:.5f} of {picks.size} draws, {len(np.unique(picks))} distinct classes")
    assert (excess < EPS).all(), (f"{what}: {(excess >= EPS).sum()} of {picks.size} draws outside the float64 band "
                                  f"of their pick, worst by {excess.max():.3g}")                           # (b)
    assert same >= 0.999, f"{what}: picks equal to float64's on {same:.5f} of {picks.size} draws"         # (c)


# ---- 1. every draw, against float64 -------------------------------------------------------------------------
@pytest.mark.parametrize("T", [0.5, 1.0])
@pytest.mark.parametrize("variant,shape,B,n_new", CASES, ids=CASE_IDS)
def test_every_draw_is_the_inverse_cdf_of_softmax_logits_over_t(variant, shape, B, n_new, T):
    Q, rf = SHAPES[shape]["input_channels"], RF[shape]
    picks, logits = _teacher_forced(variant, shape, B, n_new, T, "model")
    _check_draws(picks, logits, T, _uniforms(SEED, rf, B, n_new), Q, f"{variant} {shape} T={T}")
    if T == 1.0:
        assert len(np.unique(picks)) > Q // 8                                                            # (d)


# ---- 2. the rule changes nothing else -------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape,B,n_new", CASES, ids=CASE_IDS)
def test_rule_changes_only_the_choice(variant, shape, B, n_new):
    """logits_out does not depend on the rule, and "reference" through mvn_generate_ex is what plain mvn_generate does."""
    T, rf, Q = 1.0, RF[shape], SHAPES[shape]["input_channels"]
    picks_m, logits_m = _teacher_forced(variant, shape, B, n_new, T, "model")
    picks_r, logits_r = _teacher_forced(variant, shape, B, n_new, T, "reference")
    assert np.array_equal(logits_r.view(np.uint32), logits_m.view(np.uint32))
    # the same teacher-forced run through the old entry point
    g = _gen(shape, B, rf + n_new, variant, temperature=T, seed=SEED)
    g.samples.copy_(synthetic_indices(B, rf + n_new, Q, 4321).to(DEV))
    logits = torch.zeros(B, n_new, Q, dtype=torch.float32, device=DEV)
    choices = torch.full((B, rf + n_new), -1, dtype=torch.int32, device=DEV)
    with torch.cuda.device(g.device):
        N.check(g.lib.mvn_generate(g.dims, g.variant, g.packed.data_ptr(), g.state.data_ptr(), g.samples.data_ptr(), B,
                                   g.samples.stride(0), rf + n_new, rf + n_new, 0, rf + n_new - 1, T, SEED,
                                   logits.data_ptr(), choices.data_ptr(), rf, None,
                                   torch.cuda.current_stream(g.device).cuda_stream), "mvn_generate")
    g.check_errors()
    assert np.array_equal(choices[:, rf:].cpu().numpy(), picks_r)
    assert np.array_equal(logits.cpu().numpy().view(np.uint32), logits_r.view(np.uint32))
    assert not np.array_equal(picks_r, picks_m)  # (the two rules are different distributions on these weights)


@pytest.mark.parametrize("variant", ["FOLD", "GENERIC"])
def test_greedy_is_the_same_under_both_rules(variant):
    rf, B, n_new = RF["S64"], 4, 40
    prompt = synthetic_indices(B, rf, 256, 99).to(DEV)
    runs = []
    for sampling in ("reference", "model"):
        g = _gen("S64", B, rf + n_new, variant, temperature=0.0, sampling=sampling)
        g.prime(prompt)
        g.advance(n_new)
        g.check_errors()
        runs.append(g.samples.clone())
    assert torch.equal(runs[0], runs[1])
    assert len(torch.unique(runs[0][:, rf:])) > 1  # (a run, not a constant)


# ---- 3. frequencies against the oracle --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_step_logits():
    """The CPU oracle's logits for the step after the prompt synthetic_indices(1, rf, 256, 555) on S64."""
    sd = make_state_dict(**SHAPES["S64"], seed=3, gain=2.0, head_gain=6.0)
    pidx = synthetic_indices(1, RF["S64"], 256, 555)
    with torch.no_grad():
        return O.logits_full(sd, O.Dims(**SHAPES["S64"]), one_hot(pidx, 256))[0, :, -1].double().numpy()


@pytest.mark.parametrize("variant", ["FOLD", "GENERIC"])
def test_frequencies_match_the_oracles_softmax_of_logits_over_t(variant):
    """32 768 draws of ONE step (16 identical sequences x 2048 seeds) against softmax(oracle logits / T), T = 0.5.
    The reference rule's distribution lies about 1500 standard errors from it in the same bins."""
    T, rf, B, n_seeds = 0.5, RF["S64"], 16, 2048
    p = R.model_probs(_oracle_step_logits(), T)
    pidx = synthetic_indices(1, rf, 256, 555)
    g = _gen("S64", B, rf + 1, variant, temperature=T, seed=0, sampling="model")
    g.prime(pidx.repeat(B, 1).to(DEV))
    state0, samples0, t0 = g.state.clone(), g.samples.clone(), g.t
    draws = []
    for seed in range(n_seeds):
        g.state.copy_(state0)
        g.samples.copy_(samples0)
        g.t, g.seed = t0, seed
        g.advance(1)
        draws.append(g.samples[:, rf].clone())
    g.check_errors()
    draws = torch.cat(draws).cpu().numpy()
    n = draws.size
    assert n == 32768 and draws.min() >= 0 and draws.max() < 256
    counts = np.bincount(draws, minlength=256).astype(np.float64)
    small = n * p < 16
    assert small.any() and (~small).sum() >= 8
    pb = np.append(p[~small], p[small].sum())
    fb = np.append(counts[~small], counts[small].sum()) / n
    z = np.abs(fb - pb) / np.sqrt(pb * (1 - pb) / n)
    print(f"{variant}: worst z {z.max():.2f} over {len(pb)} bins (pooled mass {pb[-1]:.4f})")
    assert (z < 6).all(), f"{variant}: bins {np.nonzero(z >= 6)[0].tolist()} are {z[z >= 6].round(1).tolist()} standard errors out"


# ---- 4. partition independence ------------------------------------------------------------------------------------
def test_model_rule_chunked_launches_same_as_one_launch():
    rf, B, n_new = RF["S64"], 16, 60
    pidx = synthetic_indices(B, rf, 256, 99).to(DEV)
    runs = []
    for chunk in (n_new, 7, 1):
        g = _gen("S64", B, rf + n_new, "FOLD", temperature=1.0, seed=5, sampling="model")
        g.prime(pidx)
        for _ in range(0, n_new, chunk):
            g.advance(chunk)
        g.check_errors()
        runs.append(g.samples.clone())
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    assert len(torch.unique(runs[0][:, rf:])) > 32


# ---- 5. model API and grouped path --------------------------------------------------------------------------------
def test_wavenet_generate_under_the_model_rule():
    from movenet_amd.wavenet import WaveNet
    cfg, rf, B = SHAPES["S64"], RF["S64"], 2
    model = WaveNet(**cfg)
    model.load_state_dict(make_state_dict(**cfg, seed=3, gain=2.0, head_gain=6.0), strict=False)
    model.to(DEV)
    assert model.receptive_fields == rf and model.generate_sampling == "reference"
    prompt = one_hot(synthetic_indices(B, rf, 256, 11), 256).to(DEV)
    outs = {}
    for sampling in ("model", "model", "reference"):
        model.generate_sampling = sampling
        torch.manual_seed(1234)
        out = model.generate(prompt, n_samples=rf + 40, temperature=1.0)
        assert out.shape == (B, 256, rf + 40)
        assert torch.equal(out.sum(1), torch.ones(B, rf + 40, device=DEV)) and bool(((out == 0) | (out == 1)).all())
        assert torch.equal(out[:, :, :rf], prompt)
        if sampling in outs:
            assert torch.equal(out, outs[sampling])  # the same torch seed, the same samples
        outs[sampling] = out
    assert not torch.equal(outs["model"], outs["reference"])  # (the property reached the kernel)
    with pytest.raises(ValueError):
        model.generate_sampling = "top-k"
    assert model.generate_sampling == "reference"


def test_grouped_generator_draws_by_the_model_rule():
    """Groups of 8 over 20 sequences: each group is a launch of its own with its own Philox key and its own
    sequence numbering."""
    from movenet_amd.generation import GroupedGenerator
    T, rf, B, n_new = 1.0, RF["S64"], 20, 200
    gg = GroupedGenerator(**SHAPES["S64"], state_dict=_weights("S64"), batch=B, n_total=rf + n_new, device=DEV, group=8,
                          temperature=T, seed=SEED, variant=N.GEN_FOLD, sampling="model")
    assert gg.bounds == [(0, 8), (8, 16), (16, 20)]
    hist = synthetic_indices(B, rf + n_new, 256, 4321).to(DEV)
    for gi, (g, (b0, b1)) in enumerate(zip(gg.groups, gg.bounds)):
        assert g.seed == (SEED + 0x9E3779B97F4A7C15 * gi) % 2 ** 64
        choices, logits = g.teacher_forced(hist[b0:b1], logits_t0=rf)
        g.check_errors()
        _check_draws(choices[:, rf:].cpu().numpy(), logits.cpu().numpy(), T, _uniforms(g.seed, rf, b1 - b0, n_new), 256,
                     f"group {gi}")


def test_invalid_rules_are_refused():
    from movenet_amd.generation import GroupedGenerator, RingGenerator
    kw = dict(**SHAPES["S64"], state_dict=_weights("S64"), batch=2, n_total=32, device=DEV)
    with pytest.raises(ValueError, match="sampling"):
        RingGenerator(**kw, sampling="top-k")
    with pytest.raises(ValueError, match="sampling"):
        GroupedGenerator(**kw, group=1, sampling="nucleus")
    # the C ABI: nothing is launched -- samples, choices and logits stay as they were
    g = _gen("S64", 2, 32, "STREAM", temperature=1.0, seed=1)
    g.samples.copy_(synthetic_indices(2, 32, 256, 7).to(DEV))
    before = g.samples.clone()
    logits = torch.full((2, 16, 256), -7.0, dtype=torch.float32, device=DEV)
    choices = torch.full((2, 32), -1, dtype=torch.int32, device=DEV)
    with torch.cuda.device(g.device):
        rc = g.lib.mvn_generate_ex(g.dims, g.variant, g.packed.data_ptr(), g.state.data_ptr(), g.samples.data_ptr(), 2,
                                   g.samples.stride(0), 32, 16, 0, 31, 1.0, 1, logits.data_ptr(), choices.data_ptr(), 16,
                                   None, 2, torch.cuda.current_stream(g.device).cuda_stream)
    assert rc == N.MVN_ERR_BAD_ARG
    assert "sampling" in N.last_error()
    torch.cuda.synchronize()
    assert torch.equal(g.samples, before) and bool((choices == -1).all()) and bool((logits == -7.0).all())
    assert not bool(g.state.any())
