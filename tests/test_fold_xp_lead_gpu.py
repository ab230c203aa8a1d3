"""The hand-off order inside a FOLD stage: the helpers' xp' (the stream without the stage's last residual term) and
the chain's zl' reach the next stage as two halves of ONE inbox wait, and the helpers form their share of xp' over
two phases (the 16 products of Wr_0 z_0 per lane in phase 1, the cross-lane sum and the stream update in phase 2).
A value handed on in the wrong order, or a partial sum that does not survive the barrier between the phases, shows in
the results, so the results are what is checked -- at the smallest shapes that hold every class of stage:

* 3 x 3 layers: stage 0 (xp alone from the head), one middle stage, the last stage (no xp' sent) and the head;
* 10 x 1 layers over 96 steps: the queues of dilation 32 and 64 wrap, the last stage holds one real layer;
* 2 and 17 sequences, and one sequence more than the model's pipelines (65 / 49), which is where several sequences
  share a pipeline (gen_fold_kernel<true>: 32 CUs per XCD hold 8 pipelines of 4 stages, 6 of 5);
* with and without a context.

Per case: greedy samples equal STREAM's bit for bit; teacher-forced logits bit-equal between one launch and the same
run cut at an odd step (a stale xp' at a launch's first step would differ); logits within the FOLD bound of
tests/test_generate_gpu.py (2e-5 of the logit range) of the float64 oracle; the status word 0 after every launch."""
import functools

import numpy as np
import pytest
import torch

from helpers import rel_err, synthetic_indices
from movenet_amd import _native as N
from oracle import wavenet_oracle as O

pytestmark = pytest.mark.gpu
LOGIT_TOL = 2e-5
DEV = "cuda:0"
Q = C = 64
# name -> (layer_size, stack_size, new steps, batch that needs several sequences per pipeline)
SHAPES = {"3x3": (3, 3, 71, 65), "10x1": (10, 1, 96, 49)}
CASES = [pytest.param(shape, batch, cond, id=f"{shape}-B{batch if batch else 'multi'}-{'ctx' if cond else 'plain'}")
         for shape in SHAPES for batch in (2, 17, 0) for cond in (False, True)]


def _cfg(shape):
    ls, ss = SHAPES[shape][:2]
    return dict(layer_size=ls, stack_size=ss, input_channels=Q, residual_channels=C, skip_channels=C)


@functools.lru_cache(maxsize=None)
def _weights(shape):
    from movenet_amd.utils.weights import make_state_dict
    return make_state_dict(**_cfg(shape), seed=3, gain=2.0, head_gain=6.0)


@functools.lru_cache(maxsize=None)
def _weights_dev(shape):
    return {k: v.to(DEV) for k, v in _weights(shape).items()}


def _gen(shape, batch, n_total, variant, context):
    from movenet_amd.generation import RingGenerator
    g = RingGenerator(**_cfg(shape), state_dict=_weights_dev(shape), batch=batch, n_total=n_total, device=DEV,
                      variant=variant, temperature=0.0, **({} if context is None else {"context": context}))
    assert g.variant == variant
    return g


def _settled(g):
    """The launch is over and raised no status."""
    g.check_errors()
    word = g.status_word()
    if word is not None:
        assert int(word[0].item()) == 0


@functools.lru_cache(maxsize=None)
def _case(shape, batch, cond):
    """The case's inputs and FOLD's teacher-forced logits of ONE launch (shared by the tests, never written to)."""
    n_new = SHAPES[shape][2]
    B = batch or SHAPES[shape][3]
    dims = O.Dims(**_cfg(shape))
    rf = dims.receptive_fields
    assert B > 16 or batch == 2
    if not batch:  # one sequence more than the chip holds pipelines of this many stages
        assert B == 8 * (32 // (-(-dims.n_layers // 3) + 1)) + 1
    hist = synthetic_indices(B, rf + n_new, Q, 100 + B)
    ctx = None
    if cond:
        ctx = torch.from_numpy(np.random.default_rng(B).standard_normal((B, C, rf + n_new)).astype(np.float32))
    ctx_dev = None if ctx is None else ctx.to(DEV)
    g = _gen(shape, B, rf + n_new, N.GEN_FOLD, ctx_dev)
    _, logits = g.teacher_forced(hist.to(DEV), logits_t0=rf)
    _settled(g)
    return dict(B=B, rf=rf, n_new=n_new, dims=dims, hist=hist, ctx=ctx, ctx_dev=ctx_dev, logits=logits.cpu().numpy())


@pytest.mark.parametrize("shape,batch,cond", CASES)
def test_greedy_samples_equal_stream(shape, batch, cond):
    c = _case(shape, batch, cond)
    pidx = c["hist"][:, :c["rf"]].contiguous().to(DEV)
    runs = {}
    for variant in (N.GEN_STREAM, N.GEN_FOLD):
        g = _gen(shape, c["B"], c["rf"] + c["n_new"], variant, c["ctx_dev"])
        g.prime(pidx)
        g.advance(c["n_new"])
        _settled(g)
        runs[variant] = g.samples.cpu().numpy()
    differ = int((runs[N.GEN_FOLD] != runs[N.GEN_STREAM]).sum())
    print(f"{shape} B={c['B']} cond={cond}: {differ} of {runs[N.GEN_FOLD].size} samples differ, "
          f"{len(np.unique(runs[N.GEN_STREAM][:, c['rf']:]))} classes chosen")
    assert np.array_equal(runs[N.GEN_FOLD][:, :c["rf"]], c["hist"][:, :c["rf"]].numpy())
    assert differ == 0


@pytest.mark.parametrize("shape,batch,cond", CASES)
def test_teacher_forced_logits_equal_when_cut_at_an_odd_step(shape, batch, cond):
    """One launch against two: the second one's first step takes xp and zl from granules its own head and stages
    write, on queues the first one left."""
    c = _case(shape, batch, cond)
    n_total = c["rf"] + c["n_new"]
    cut = c["rf"] + 37  # odd, inside the steps whose logits are kept
    assert cut % 2 == 1 and c["rf"] < cut < n_total - 1
    g = _gen(shape, c["B"], n_total, N.GEN_FOLD, c["ctx_dev"])
    g.reset()
    g.samples.copy_(c["hist"].to(DEV).to(torch.int32))
    logits = torch.zeros(c["B"], c["n_new"], Q, dtype=torch.float32, device=DEV)
    choices = torch.full((c["B"], n_total), -1, dtype=torch.int32, device=DEV)
    for t0, t1 in ((0, cut), (cut, n_total - 1)):
        g._run(t0, t1, n_total, logits, choices, c["rf"])
        _settled(g)
    got = logits.cpu().numpy()
    differ = int((got.view(np.uint32) != c["logits"].view(np.uint32)).sum())
    print(f"{shape} B={c['B']} cond={cond}: {differ} of {got.size} logits differ between one launch and two")
    assert differ == 0


@pytest.mark.parametrize("shape,batch,cond", CASES)
def test_teacher_forced_logits_against_float64(shape, batch, cond):
    c = _case(shape, batch, cond)
    sd64 = {k: v.double() for k, v in _weights(shape).items()}
    x = torch.nn.functional.one_hot(c["hist"].long(), Q).permute(0, 2, 1).double()
    with torch.no_grad():
        # oracle column s = the logits after consuming time s + rf - 1, which pick time s + rf
        want = O.forward(sd64, c["dims"], x, output_unnormalized=False, remove_last=False,
                         context=None if c["ctx"] is None else c["ctx"].double())[:, :, :c["n_new"]]
    want = want.permute(0, 2, 1).numpy()
    assert want.shape == c["logits"].shape == (c["B"], c["n_new"], Q)
    err = rel_err(c["logits"], want)
    print(f"{shape} B={c['B']} cond={cond}: logit error {err:.3e} of the range")
    assert np.isfinite(c["logits"]).all()
    assert err <= LOGIT_TOL
