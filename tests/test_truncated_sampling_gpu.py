"""GPU: top-k / top-p truncation of a sampled generator step (mvn_generate_trunc, include/movenet_hip.h) on all five
generator kernels, on the shapes, weights and nine cases of tests/test_model_sampling_gpu.py.

Every draw is checked against float64 (tests/truncation_reference.py) computed from the kernel's OWN logits and the
exact Philox uniform: the kept set, the inverse CDF over the truncated weights, and the pick.

Bounds.  A step is CLEAR unless its float64 kept set hinges on rounding (truncation_reference.unclear: the fp32 sum
against p S within 2^-14, the threshold weight within 2^-18 of its neighbour).  On every step the pick lies in the
WIDE kept set (p (1 + 2^-14), near-ties kept).  On clear steps: the pick lies in the kept set, inside the float64 band
of the truncated CDF within eps = 2^-14 (a 256-term fp32 running sum, tests/test_model_sampling_gpu.py), and equals
float64's pick on >= 99.9 % of them (the project's figure for draws within rounding of a CDF edge).  Unclear steps
are at most 10 % of a top-p case (worst share from the oracle's logits on the CPU: 4.8 %, S64 at T = 1, p = 0.9)
and at most 1 % by top-k's criterion (0.04 %).  Measured on an MI355X from the kernels' own logits: top-p 4.82 % at
worst (S64, T = 1, p = 0.9, every fp32 kernel; PIPE_F16 on S128: 3.21 %), top-k 0.06 % (reference rule, k = 8)."""
import math

import numpy as np
import pytest
import torch

import sampling_reference as R
import test_model_sampling_gpu as M
import truncation_reference as TR
from helpers import one_hot, synthetic_indices
from movenet_amd import _native as N
from movenet_amd.utils.weights import make_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -14
SEED = 77
SHAPES, RF, VARIANTS, CASES, CASE_IDS = M.SHAPES, M.RF, M.VARIANTS, M.CASES, M.CASE_IDS
# (temperature, top_k, top_p)
SETTINGS = [(1.0, 8, 1.0), (1.0, 40, 1.0), (1.0, 0, 0.9), (0.5, 0, 0.5), (1.0, 40, 0.9)]
# one case per kernel, for the checks that are about the entry point rather than the draw
ONE_PER_VARIANT = [("GENERIC", "S16"), ("STREAM", "S64"), ("PIPE", "S64"), ("FOLD", "S64q"), ("PIPE_F16", "S128")]
WEIGHTS = {"model": TR.model_weights, "reference": TR.reference_weights}


def _gen(shape, batch, n_total, variant, temperature=0.0, seed=0, sampling="model", top_k=0, top_p=1.0):
    from movenet_amd.generation import RingGenerator
    g = RingGenerator(**SHAPES[shape], state_dict=M._weights(shape), batch=batch, n_total=n_total, device=DEV,
                      variant=VARIANTS[variant] if isinstance(variant, str) else variant, temperature=temperature,
                      seed=seed, sampling=sampling, top_k=top_k, top_p=top_p)
    assert g.rf == RF[shape]
    return g


def _teacher_forced(variant, shape, B, n_new, T, top_k, top_p, sampling="model"):
    """(picks (B, n_new) for times rf .. rf + n_new - 1, logits (B, n_new, Q)) of one teacher-forced run, as numpy."""
    rf, Q = RF[shape], SHAPES[shape]["input_channels"]
    g = _gen(shape, B, rf + n_new, variant, temperature=T, seed=SEED, sampling=sampling, top_k=top_k, top_p=top_p)
    hist = synthetic_indices(B, rf + n_new, Q, 4321).to(DEV)
    choices, logits = g.teacher_forced(hist, logits_t0=g.rf)
    g.check_errors()
    return choices[:, rf:].cpu().numpy(), logits.cpu().numpy()


def _take(mask, picks):
    return np.take_along_axis(mask, picks.astype(np.int64)[..., None], axis=-1)[..., 0]


def _check_truncated_draws(picks, logits, T, top_k, top_p, uniform, Q, what, sampling="model"):
    """Check 1 of this file's header on every draw of a run; returns the number of distinct picks."""
    assert logits.shape == picks.shape + (Q,) and np.isfinite(logits).all()
    assert picks.min() >= 0 and picks.max() < Q, f"{what}: picks outside [0, {Q})"
    w = WEIGHTS[sampling](logits, T)
    kept, wide = TR.kept_set(w, top_k, top_p), TR.wide_kept_set(w, top_k, top_p)
    unclear_k, unclear_p = TR.unclear(w, top_k, top_p)
    clear = ~(unclear_k | unclear_p)
    cdf = TR.truncated_cdf(w, kept)
    excess = R.band_excess(picks, cdf, uniform)[clear]
    same = (picks == R.inverse_cdf_picks(cdf, uniform))[clear].mean()
    in_kept, in_wide = _take(kept, picks), _take(wide, picks)
    distinct = len(np.unique(picks))
    print(f"{what}: unclear share top-k {unclear_k.mean():.5f}, top-p {unclear_p.mean():.5f}; kept classes per step "
          f"{kept.sum(-1).min()} .. {kept.sum(-1).max()}; picks outside the wide set {(~in_wide).sum()}, outside the "
          f"kept set on clear steps {(~in_kept[clear]).sum()}; worst excess over the float64 band "
          f"{excess.max():.3g} (eps {EPS:.3g}); equal to float64's pick on {same:.5f} of {clear.sum()} clear draws; "
          f"{distinct} distinct classes")
    assert in_wide.all(), f"{what}: {(~in_wide).sum()} of {picks.size} picks outside the wide kept set"
    assert in_kept[clear].all(), f"{what}: {(~in_kept[clear]).sum()} picks of clear steps outside the kept set"
    assert (excess < EPS).all(), (f"{what}: {(excess >= EPS).sum()} of {clear.sum()} clear draws outside the float64 "
                                  f"band of their pick, worst by {excess.max():.3g}")
    assert same >= 0.999, f"{what}: picks equal to float64's on {same:.5f} of {clear.sum()} clear draws"
    assert unclear_k.mean() <= 0.01, f"{what}: {unclear_k.mean():.4f} of the steps are unclear for top-k"
    assert (unclear_k | unclear_p).mean() <= 0.10, f"{what}: {(~clear).mean():.4f} of the steps are unclear"
    assert distinct > 1, f"{what}: every draw picked class {picks.flat[0]}"
    return distinct


def _setting_id(s):
    return f"T{s[0]}-k{s[1]}-p{s[2]}"


# ---- 1. every draw, against float64 ---------------------------------------------------------------------------
_DRAW_PARAMS = [pytest.param(*c, *s, id=f"{i}-{_setting_id(s)}") for c, i in zip(CASES, CASE_IDS) for s in SETTINGS
                if s[1] < SHAPES[c[1]]["input_channels"]]


@pytest.mark.parametrize("variant,shape,B,n_new,T,top_k,top_p", _DRAW_PARAMS)
def test_every_draw_comes_from_the_truncated_distribution(variant, shape, B, n_new, T, top_k, top_p):
    Q, rf = SHAPES[shape]["input_channels"], RF[shape]
    picks, logits = _teacher_forced(variant, shape, B, n_new, T, top_k, top_p)
    distinct = _check_truncated_draws(picks, logits, T, top_k, top_p, M._uniforms(SEED, rf, B, n_new), Q,
                                      f"{variant} {shape} T={T} k={top_k} p={top_p}")
    if shape == "S64" and (T, top_k, top_p) == (1.0, 0, 0.9):
        assert distinct > 20


def test_truncation_applies_under_the_reference_rule_too():
    """FOLD, S64, T = 1, k = 8 on the reference's double softmax.  (top-k, because that rule's weights are close to
    uniform: its 8 largest are as distinct as the model's probabilities, while a nucleus threshold would fall among
    hundreds of weights that agree to within 1e-6.)"""
    variant, shape, B, n_new = "FOLD", "S64", 16, 700
    picks, logits = _teacher_forced(variant, shape, B, n_new, 1.0, 8, 1.0, sampling="reference")
    _check_truncated_draws(picks, logits, 1.0, 8, 1.0, M._uniforms(SEED, RF[shape], B, n_new), 256,
                           "FOLD S64 reference rule T=1.0 k=8", sampling="reference")
    assert len(np.unique(picks)) > 8  # (the 8 kept classes change from step to step)


# ---- 2. off means off -------------------------------------------------------------------------------------------
def _abi_teacher_forced(g, hist, T, sampling, trunc):
    """One teacher-forced run straight through the C ABI: mvn_generate_ex (trunc None) or mvn_generate_trunc
    (trunc = (top_k, top_p)); (choices (B, n_new), logits bits (B, n_new, Q)) as numpy."""
    B, n_total, rf = g.batch, g.n_total, g.rf
    g.reset()
    g.samples.copy_(hist)
    logits = torch.zeros(B, n_total - rf, g.Q, dtype=torch.float32, device=DEV)
    choices = torch.full((B, n_total), -1, dtype=torch.int32, device=DEV)
    head = (g.dims, g.variant, g.packed.data_ptr(), g.state.data_ptr(), g.samples.data_ptr(), B, g.samples.stride(0),
            n_total, n_total, 0, n_total - 1, T, SEED, logits.data_ptr(), choices.data_ptr(), rf, None,
            N.sampling_rule(sampling))
    stream = torch.cuda.current_stream(g.device).cuda_stream
    with torch.cuda.device(g.device):
        if trunc is None:
            N.check(g.lib.mvn_generate_ex(*head, stream), "mvn_generate_ex")
        else:
            N.check(g.lib.mvn_generate_trunc(*head, *trunc, stream), "mvn_generate_trunc")
    g.check_errors()
    return choices[:, rf:].cpu().numpy(), logits.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("variant,shape", ONE_PER_VARIANT, ids=[v for v, _ in ONE_PER_VARIANT])
def test_off_is_bit_equal_to_generate_ex_and_greedy_ignores_the_knobs(variant, shape):
    rf, Q, B, n_new = RF[shape], SHAPES[shape]["input_channels"], 4, 120
    g = _gen(shape, B, rf + n_new, variant)
    hist = synthetic_indices(B, rf + n_new, Q, 4321).to(DEV).to(torch.int32)
    for sampling in ("reference", "model"):
        picks, bits = _abi_teacher_forced(g, hist, 1.0, sampling, None)
        assert len(np.unique(picks)) > 1
        for trunc in ((0, 1.0), (Q, 1.0)):
            picks_t, bits_t = _abi_teacher_forced(g, hist, 1.0, sampling, trunc)
            assert np.array_equal(picks_t, picks), f"{sampling} {trunc}"
            assert np.array_equal(bits_t, bits), f"{sampling} {trunc}"
        # (and the knobs do reach the kernel: k = 2 draws differently, from the same logits)
        picks_2, bits_2 = _abi_teacher_forced(g, hist, 1.0, sampling, (2, 1.0))
        assert not np.array_equal(picks_2, picks) and np.array_equal(bits_2, bits)
    greedy, bits = _abi_teacher_forced(g, hist, 0.0, "model", None)
    greedy_t, bits_t = _abi_teacher_forced(g, hist, 0.0, "model", (8, 0.9))
    assert np.array_equal(greedy_t, greedy) and np.array_equal(bits_t, bits)


# ---- 3. top_k = 1 is the arg-max ----------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape,B,n_new", CASES, ids=CASE_IDS)
def test_top_k_one_picks_the_largest_logit(variant, shape, B, n_new):
    picks, logits = _teacher_forced(variant, shape, B, n_new, 1.0, 1, 1.0)
    w = -np.sort(-TR.model_weights(logits, 1.0), axis=-1)
    distinct = (w[..., 0] - w[..., 1]) > TR.TIE_EPS * w[..., 0]  # the top two differ by more than 2^-18 relative
    assert distinct.mean() > 0.99
    assert np.array_equal(picks[distinct], logits.astype(np.float64).argmax(-1)[distinct])
    assert len(np.unique(picks)) > 1


# ---- 4. launch partition and turns --------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["FOLD", "GENERIC"])
def test_chunked_launches_same_as_one_launch(variant):
    rf, B, n_new = RF["S64"], 16, 60
    pidx = synthetic_indices(B, rf, 256, 99).to(DEV)
    runs = []
    for chunk in (n_new, 7, 1):
        g = _gen("S64", B, rf + n_new, variant, temperature=1.0, seed=5, top_k=8, top_p=0.9)
        g.prime(pidx)
        for _ in range(0, n_new, chunk):
            g.advance(chunk)
        g.check_errors()
        runs.append(g.samples.clone())
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    assert len(torch.unique(runs[0][:, rf:])) > 8


@pytest.mark.parametrize("variant,shape", [("PIPE", "S64"), ("FOLD", "S64"), ("PIPE_F16", "S128")],
                         ids=["PIPE", "FOLD", "PIPE_F16"])
def test_more_sequences_than_pipelines(variant, shape):
    """Three sequences more than the launch has pipelines: the head stages serve several sequences in turn."""
    rf, Q, n_new, (T, top_k, top_p) = RF[shape], 256, 100, (1.0, 40, 0.9)
    pipes = N.lib().mvn_gen_launch_pipelines(N.make_dims(**SHAPES[shape]), VARIANTS[variant], 1 << 20)
    assert pipes >= 1
    B = pipes + 3
    picks, logits = _teacher_forced(variant, shape, B, n_new, T, top_k, top_p)
    _check_truncated_draws(picks, logits, T, top_k, top_p, M._uniforms(SEED, rf, B, n_new), Q,
                           f"{variant} {shape} {B} sequences on {pipes} pipelines")


# ---- 5. free run through the model API and the grouped path ------------------------------------------------------
def _check_free_run(samples, g, rf, T, top_k, top_p, what):
    """``samples`` (B, n_total) generated freely by a launch with g's seed: a teacher-forced pass over them must draw
    them again, each inside the wide kept set of its step."""
    choices, logits = g.teacher_forced(samples, logits_t0=rf)
    g.check_errors()
    again, own = choices[:, rf:].cpu().numpy(), samples[:, rf:].cpu().numpy()
    same = (again == own).mean()
    wide = TR.wide_kept_set(TR.model_weights(logits.cpu().numpy(), T), top_k, top_p)
    print(f"{what}: {same:.5f} of {own.size} free-run draws reproduced, {(~_take(wide, own)).sum()} outside the wide "
          f"kept set, {len(np.unique(own))} distinct classes")
    assert same >= 0.999
    assert _take(wide, own).all()
    assert len(np.unique(own)) > 1


def test_wavenet_generate_with_truncation():
    from movenet_amd.wavenet import WaveNet
    cfg, rf, B, n_new, (T, top_k, top_p) = SHAPES["S64"], RF["S64"], 2, 300, (1.0, 8, 0.9)
    model = WaveNet(**cfg)
    model.load_state_dict(make_state_dict(**cfg, seed=3, gain=2.0, head_gain=6.0), strict=False)
    model.to(DEV)
    assert (model.generate_top_k, model.generate_top_p) == (0, 1.0)
    model.generate_sampling, model.generate_top_k, model.generate_top_p = "model", top_k, top_p
    prompt = one_hot(synthetic_indices(B, rf, 256, 11), 256).to(DEV)
    torch.manual_seed(1234)
    out = model.generate(prompt, n_samples=rf + n_new, temperature=T)
    assert out.shape == (B, 256, rf + n_new) and torch.equal(out[:, :, :rf], prompt)
    assert torch.equal(out.sum(1), torch.ones(B, rf + n_new, device=DEV))
    torch.manual_seed(1234)
    seed = int(torch.empty((), dtype=torch.int64).random_().item())  # the draw generate() keys its launch with
    g = _gen("S64", B, rf + n_new, N.GEN_AUTO, temperature=T, seed=seed, top_k=top_k, top_p=top_p)
    _check_free_run(out.argmax(1).to(torch.int32), g, rf, T, top_k, top_p, "WaveNet.generate")
    # off again: a different run from the same torch seed
    model.generate_top_k, model.generate_top_p = 0, 1.0
    torch.manual_seed(1234)
    assert not torch.equal(model.generate(prompt, n_samples=rf + n_new, temperature=T), out)


def test_grouped_generator_with_truncation():
    from movenet_amd.generation import GroupedGenerator
    rf, B, n_new, (T, top_k, top_p) = RF["S64"], 5, 300, (1.0, 8, 0.9)
    gg = GroupedGenerator(**SHAPES["S64"], state_dict=M._weights("S64"), batch=B, n_total=rf + n_new, device=DEV,
                          group=2, temperature=T, seed=SEED, variant=N.GEN_FOLD, sampling="model", top_k=top_k,
                          top_p=top_p)
    assert gg.bounds == [(0, 2), (2, 4), (4, 5)]
    assert all((g.top_k, g.top_p) == (top_k, top_p) for g in gg.groups)
    gg.prime(synthetic_indices(B, rf, 256, 11).to(DEV))
    gg.advance(n_new)
    gg.check_errors()
    free = gg.samples.clone()
    for gi, (g, (b0, b1)) in enumerate(zip(gg.groups, gg.bounds)):
        _check_free_run(free[b0:b1], g, rf, T, top_k, top_p, f"group {gi}")


# ---- 6. refusals ----------------------------------------------------------------------------------------------
BAD = [(-1, 1.0), (0, 0.0), (0, -0.1), (0, 1.5), (0, math.nan)]


def test_bad_values_are_refused_by_the_c_abi_before_anything_is_touched():
    g = _gen("S64", 2, 32, "STREAM", temperature=1.0, seed=1)
    g.samples.copy_(synthetic_indices(2, 32, 256, 7).to(DEV))
    g.state.fill_(3.25)
    logits = torch.full((2, 16, 256), -7.0, dtype=torch.float32, device=DEV)
    choices = torch.full((2, 32), -1, dtype=torch.int32, device=DEV)
    samples0, state0 = g.samples.clone(), g.state.clone()
    for top_k, top_p in BAD:
        with torch.cuda.device(g.device):
            rc = g.lib.mvn_generate_trunc(g.dims, g.variant, g.packed.data_ptr(), g.state.data_ptr(),
                                          g.samples.data_ptr(), 2, g.samples.stride(0), 32, 16, 0, 31, 1.0, 1,
                                          logits.data_ptr(), choices.data_ptr(), 16, None, N.SAMPLE_MODEL, top_k, top_p,
                                          torch.cuda.current_stream(g.device).cuda_stream)
        assert rc == N.MVN_ERR_BAD_ARG, (top_k, top_p)
        assert "top_k" in N.last_error() and "top_p" in N.last_error()
        torch.cuda.synchronize()
        assert torch.equal(g.samples, samples0) and torch.equal(g.state, state0)
        assert bool((choices == -1).all()) and bool((logits == -7.0).all())


def test_bad_values_are_refused_by_the_python_layers():
    from movenet_amd.generation import GroupedGenerator, RingGenerator
    from movenet_amd.wavenet import WaveNet
    kw = dict(**SHAPES["S64"], state_dict=M._weights("S64"), batch=2, n_total=32, device=DEV)
    model = WaveNet(**SHAPES["S64"])
    for top_k, top_p in BAD:
        with pytest.raises(ValueError, match="top_[kp]"):
            RingGenerator(**kw, top_k=top_k, top_p=top_p)
        with pytest.raises(ValueError, match="top_[kp]"):
            GroupedGenerator(**kw, group=1, top_k=top_k, top_p=top_p)
        with pytest.raises(ValueError, match="top_[kp]"):
            model.generate_top_k, model.generate_top_p = top_k, top_p
        assert (model.generate_top_k, model.generate_top_p) == (0, 1.0)
