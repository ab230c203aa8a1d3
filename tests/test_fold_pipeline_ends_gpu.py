"""The ends of the FOLD pipeline: stage 0 has a form of its own -- it takes the stream alone from the head (no zl,
no skip sum: there is no previous layer) and forms none of the products against them -- and the last layer stage
feeds the head.  Every case compares gen_fold_kernel with the GENERIC kernel at a shape that makes those stages
special (one stage that is both, a partial last stage, queue wraps, chunked launches, several sequences per
pipeline, conditioning, sampling), under the tolerances tests/test_generate_gpu.py uses for FOLD: teacher-forced
logits within 2e-5 of the logit range, greedy class indices equal."""
import numpy as np
import pytest
import torch

from helpers import rel_err, synthetic_indices
from movenet_amd import _native as N

pytestmark = pytest.mark.gpu
LOGIT_TOL = 2e-5
DEV = "cuda:0"
CFG2 = dict(layer_size=10, stack_size=3, input_channels=256, residual_channels=64, skip_channels=64)


def _cfg(layer_size, stack_size):
    return dict(layer_size=layer_size, stack_size=stack_size, input_channels=256, residual_channels=64,
                skip_channels=64)


def _rf(cfg):
    # prompt length: at least the receptive field (movenet/wavenet.py:125-134); config 2: 3072
    return sum(2 ** (l % cfg["layer_size"]) for l in range(cfg["layer_size"] * cfg["stack_size"])) + max(2, cfg["stack_size"])


def _weights(cfg, seed):
    from movenet_amd.utils.weights import make_state_dict
    return {k: v.to(DEV) for k, v in make_state_dict(**cfg, seed=seed, gain=2.0, head_gain=6.0).items()}


def _gen(cfg, sd, batch, n_total, variant, temperature=0.0, seed=0, context=None):
    from movenet_amd.generation import RingGenerator
    g = RingGenerator(**cfg, state_dict=sd, batch=batch, n_total=n_total, device=DEV, variant=variant,
                      temperature=temperature, seed=seed, **({} if context is None else {"context": context}))
    assert g.variant == variant
    return g


def _free_run(cfg, sd, pidx, n_new, variant, chunks=None, context=None):
    g = _gen(cfg, sd, pidx.shape[0], pidx.shape[1] + n_new, variant, context=context)
    g.prime(pidx)
    for n in (chunks or [n_new]):
        g.advance(n)
    g.check_errors()
    return g.samples.clone()


def _check_against_generic(cfg, sd, B, n_new, idx_seed, context=None):
    """Greedy free runs equal; on a random teacher-forced history (a tiny model's own run settles on one class) the
    logits within LOGIT_TOL of the logit range and the greedy choices equal."""
    rf = _rf(cfg)
    hist = synthetic_indices(B, rf + n_new, 256, idx_seed).to(DEV)
    pidx = hist[:, :rf].contiguous()
    ref = _free_run(cfg, sd, pidx, n_new, N.GEN_GENERIC, context=context)
    got = _free_run(cfg, sd, pidx, n_new, N.GEN_FOLD, context=context)
    logits, picks = {}, {}
    for variant in (N.GEN_GENERIC, N.GEN_FOLD):
        g = _gen(cfg, sd, B, rf + n_new, variant, context=context)
        ch, lg = g.teacher_forced(hist, logits_t0=rf)
        g.check_errors()
        logits[variant], picks[variant] = lg.cpu().numpy(), ch[:, rf:].cpu().numpy()
    err = rel_err(logits[N.GEN_FOLD], logits[N.GEN_GENERIC])
    print(f"L={cfg['layer_size'] * cfg['stack_size']} B={B} steps={n_new}: logit error {err:.3e} of the range, "
          f"{int((got != ref).sum().item())} free-run and {int((picks[N.GEN_FOLD] != picks[N.GEN_GENERIC]).sum())} "
          f"teacher-forced indices differ, {len(np.unique(picks[N.GEN_GENERIC]))} classes chosen")
    assert err < LOGIT_TOL
    assert torch.equal(got, ref)
    assert np.array_equal(picks[N.GEN_FOLD], picks[N.GEN_GENERIC])
    return ref


@pytest.mark.parametrize("L", [1, 2, 3])
def test_stage0_is_also_the_last_layer_stage(L):
    """L <= 3: ONE layer stage, which takes the head's stream alone AND feeds the head."""
    cfg = _cfg(L, 1)
    _check_against_generic(cfg, _weights(cfg, 3), B=3, n_new=200, idx_seed=21)


@pytest.mark.parametrize("L", [4, 7])
def test_partial_last_stage_feeds_the_head(L):
    """L = 4, 7: the last layer stage holds ONE real layer (the other two are packed as zeros)."""
    cfg = _cfg(L, 1)
    _check_against_generic(cfg, _weights(cfg, 3), B=3, n_new=400, idx_seed=22)


def test_config2_over_a_wrap_of_every_queue_and_in_two_launches():
    """The config-2 shape over 1100 steps (the longest dilation queue holds 512 entries: every queue wraps, the
    longest twice), as one launch and as two chunked ones (t_begin > 0: the second launch's prologue pops what the
    first one's last step pushed)."""
    sd = _weights(CFG2, 1)
    B, n_new = 16, 1100
    ref = _check_against_generic(CFG2, sd, B, n_new, idx_seed=1234)
    pidx = ref[:, :_rf(CFG2)].contiguous()
    two = _free_run(CFG2, sd, pidx, n_new, N.GEN_FOLD, chunks=[537, 563])
    assert torch.equal(two, ref)


def test_forty_sequences_in_turn():
    """40 sequences on 16 pipelines: gen_fold_kernel<true>, the last round half empty."""
    _check_against_generic(CFG2, _weights(CFG2, 1), B=40, n_new=48, idx_seed=77)


def test_conditioned_run():
    sd = _weights(CFG2, 1)
    assert any(".context_conv_" in k for k in sd)
    B, n_new = 3, 40
    ctx = torch.from_numpy(np.random.default_rng(9).standard_normal((B, 64, _rf(CFG2) + n_new)).astype(np.float32))
    _check_against_generic(CFG2, sd, B, n_new, idx_seed=5, context=ctx.to(DEV))


def test_sampled_draws_equal_generic():
    """Temperature 1 on one teacher-forced history (a differing draw cannot change later inputs): the same class
    on >= 99.9 % of 11 200 draws, as test_sampler_same_draws_on_generic_stream_pipe asks of every pair of kernels."""
    sd = _weights(CFG2, 3)
    rf, B, n_new = _rf(CFG2), 16, 700
    hist = synthetic_indices(B, rf + n_new, 256, 4321).to(DEV)
    picks = {}
    for variant in (N.GEN_GENERIC, N.GEN_FOLD):
        g = _gen(CFG2, sd, B, rf + n_new, variant, temperature=1.0, seed=77)
        choices, _ = g.teacher_forced(hist, logits_t0=rf)
        g.check_errors()
        picks[variant] = choices[:, rf:].cpu().numpy()
    same = (picks[N.GEN_FOLD] == picks[N.GEN_GENERIC]).mean()
    print(f"sampled draws equal on {same:.5f} of {picks[N.GEN_FOLD].size}")
    assert picks[N.GEN_FOLD].size >= 10000 and same >= 0.999
    assert len(np.unique(picks[N.GEN_FOLD])) > 32  # samples, not the arg-max
