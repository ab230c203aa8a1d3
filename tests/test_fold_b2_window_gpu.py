"""GPU: the FOLD generator computes what it computed BEFORE its chain waves moved (Wc_2 Wr_0) z_0 from phase 1 of a
layer stage into phase 2 (generate_fold.hip: z_0 stays in registers across the phase-1 barrier, and the product issues
behind the four LDS reads of z_1, while they are in flight).

Only WHEN the 16 packed FMAs issue changed -- same operands, same four accumulators, same order of sums -- so the
yardstick is bit identity: SHA-256 hashes of ``logits_out``, ``choices_out`` and ``samples``, recorded on an MI355X from
a library built at the commit BEFORE the change, fde089c (tests/golden/fold_b2_window_sha256.json; its header names
that commit too).  The FOLD variant is forced, the weights are make_state_dict(seed=3, gain=2.0, head_gain=6.0).

* ``config2``: 10 x 3 layers, C = K = 64, Q = 256, 2 sequences, one launch over the prompt, 48 teacher-forced steps
  (a random history) and 48 free greedy steps; logits and choices of the 96 steps and the samples against the recording,
  and the samples equal STREAM's.  Stage 0 (no previous layer), eight middle stages and the last stage;
* ``two-by-two``: 2 x 2 layers, the same run.  Its second layer stage has ONE real layer and two missing ones: their
  B2' is packed as zeros and b2 has to be a clean 0.  Every buffer the generator allocates without filling comes out
  of memory that held NaNs (blocks of NaNs given back to the caching allocator just before), logits_out starts as NaNs;
* ``seventeen``: 17 sequences on 16 pipelines, 40 free steps -- one pipeline serves two sequences in turn (the MULTI
  form: z_0 of one sequence's turn must not reach the next one's phase 2); samples equal STREAM's, and the recording;
* ``seq``: 2 x 2 layers, 3 sequences, 32 sampled steps through the per-sequence launch (own temperatures, one
  truncated row, permuted Philox rows);
* ``guided``: 2 x 2 layers, one pair through mvn_generate_guided (two turns per step), 32 steps;
* ``split``: ``config2``'s shape, 40 free greedy steps in launches of 13 + 27 against one launch of 40.

``check_errors()`` is clean after every launch sequence.  No case makes a hand-off time out.

The fixture is only worth something recorded from the parent's library: --record refuses to run unless MOVENET_HIP_LIB
names the library it is to record from, and wants the commit that library was built at.

    MOVENET_HIP_LIB=<library built at that commit> python tests/test_fold_b2_window_gpu.py --record <commit>
"""
import functools
import hashlib
import json
import os
import sys

import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from movenet_amd import _native as N
from movenet_amd.generation import RingGenerator
from movenet_amd.utils.weights import make_state_dict, synthetic_indices

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fold_b2_window_sha256.json")
DEV = "cuda:0"
C = 64
CONFIG2, TWO_BY_TWO = (10, 3, 256), (2, 2, 256)


def _cfg(layer_size, stack_size, Q):
    return dict(layer_size=layer_size, stack_size=stack_size, input_channels=Q, residual_channels=C, skip_channels=C)


@functools.lru_cache(maxsize=None)
def _weights(layer_size, stack_size, Q):
    sd = make_state_dict(**_cfg(layer_size, stack_size, Q), seed=3, gain=2.0, head_gain=6.0)
    return {k: v.to(DEV) for k, v in sd.items()}


def _rf(shape):
    return N.check(N.lib().mvn_receptive_fields(N.make_dims(**_cfg(*shape))), "mvn_receptive_fields")


def _gen(shape, batch, n_total, variant=N.GEN_FOLD, **kw):
    kw.setdefault("temperature", 0.0)
    g = RingGenerator(**_cfg(*shape), state_dict=_weights(*shape), batch=batch, n_total=n_total, device=DEV,
                      variant=variant, **kw)
    assert g.variant == variant
    return g


def _settled(g):
    g.check_errors()
    word = g.status_word()
    assert word is None or int(word[0].item()) == 0


def _sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def _poison_free_memory():
    """Blocks of NaNs of several sizes, given back to the caching allocator: what is allocated next without being
    filled (torch.empty: the packed weights, a context buffer) starts as NaNs."""
    junk = [torch.full((n,), float("nan"), dtype=torch.float32, device=DEV) for n in (1 << 24, 1 << 22, 1 << 20, 1 << 16, 1 << 12)]
    torch.cuda.synchronize()
    del junk


def _forced_then_free(shape, batch, variant=N.GEN_FOLD, forced=48, free=48, poison=False):
    """ONE launch from t = 0: the prompt (rf samples) and ``forced`` more steps are fed a random history, ``free``
    greedy steps follow; logits and choices of the forced + free steps."""
    rf = _rf(shape)
    if poison:
        _poison_free_memory()
    g = _gen(shape, batch, rf + forced + free, variant=variant)
    given = rf + forced
    g.reset()
    g.samples_all.zero_()
    g.samples[:, :given] = synthetic_indices(batch, given, shape[2], 100 + batch + shape[2]).to(DEV)
    logits = torch.full((g.nrows, forced + free, g.Q), float("nan") if poison else 0.0, dtype=torch.float32, device=DEV)
    choices = torch.full((g.nrows, g.n_total), -1, dtype=torch.int32, device=DEV)
    g._run(0, g.n_total - 1, given, logits, choices, rf)
    _settled(g)
    assert bool(torch.isfinite(logits).all().item())
    return {"logits": _sha(logits), "choices": _sha(choices[:, rf:]), "samples": _sha(g.samples_all)}, g.samples_all.clone()


def _greedy(shape, poison):
    got, samples = _forced_then_free(shape, 2, poison=poison)
    _, want = _forced_then_free(shape, 2, variant=N.GEN_STREAM)
    assert torch.equal(samples, want), "FOLD's greedy samples differ from STREAM's"
    return got


def _free_run(g, parts, out, prompt=None):
    """Free run of sum(parts) steps from a prompt of ``prompt`` (default: rf) samples, one launch per part; ``out``:
    with logits_out / choices_out of every step (one launch).  Returns the hashes and the samples."""
    P = prompt or g.rf
    assert P + sum(parts) == g.n_total
    g.prime(synthetic_indices(g.batch, P, g.Q, 4321).to(DEV))
    got = {}
    if out:
        assert len(parts) == 1
        logits = torch.zeros(g.nrows, parts[0], g.Q, dtype=torch.float32, device=DEV)
        choices = torch.full((g.nrows, g.n_total), -1, dtype=torch.int32, device=DEV)
        g._run(g.t, g.n_total - 1, P, logits, choices, P)
        _settled(g)
        assert bool(torch.isfinite(logits).all().item())
        got = {"logits": _sha(logits), "choices": _sha(choices[:, P:])}
    else:
        for n in parts:
            g.advance(n)
        _settled(g)
    got["samples"] = _sha(g.samples_all)
    return got, g.samples_all.clone()


def _seventeen():
    n = _rf(CONFIG2) + 40
    got, samples = _free_run(_gen(CONFIG2, 17, n), (40,), True)
    _, want = _free_run(_gen(CONFIG2, 17, n, variant=N.GEN_STREAM), (40,), False)
    assert torch.equal(samples, want), "FOLD's greedy samples (two turns on one pipeline) differ from STREAM's"
    return got


def _seq():
    per_seq = dict(temperature=[1.0, 0.7, 1.0], top_k=[0, 40, 0], top_p=[1.0, 0.9, 1.0], seed=[5, 6, 7], rows=[2, 0, 1])
    return _free_run(_gen(TWO_BY_TWO, 3, _rf(TWO_BY_TWO) + 32, sampling="model", **per_seq), (32,), True)[0]


def _guided():
    vec = torch.randn(1, C, generator=torch.Generator().manual_seed(17)).to(DEV)
    g = _gen(TWO_BY_TWO, 1, 33, temperature=[0.0], top_k=[0], top_p=[1.0], seed=[9], global_context=vec, guidance=2.0)
    assert g.nrows == 2
    return _free_run(g, (32,), True, prompt=1)[0]  # (a one-sample prompt: primed by stepping, both rows of the pair)


def _split():
    n = _rf(CONFIG2) + 40
    one, _ = _free_run(_gen(CONFIG2, 2, n), (40,), False)
    two, _ = _free_run(_gen(CONFIG2, 2, n), (13, 27), False)
    assert one == two  # launches of 13 + 27 steps pick what one launch of 40 picks
    return one


CASES = {
    "config2": lambda: _greedy(CONFIG2, False),
    "two-by-two": lambda: _greedy(TWO_BY_TWO, True),
    "seventeen": _seventeen,
    "seq": _seq,
    "guided": _guided,
    "split": _split,
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_outputs_equal_the_recording(case):
    with open(FIXTURE) as f:
        want = json.load(f)["cases"][case]
    got = CASES[case]()
    print(f"{case}: " + ", ".join(f"{k} {'ok' if got[k] == want.get(k) else 'DIFFERS'}" for k in sorted(got)))
    assert got == want


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record" and os.environ.get("MOVENET_HIP_LIB"), __doc__
    out = {"recorded_from_commit": sys.argv[2],
           "what": "SHA-256 of logits_out / choices_out / samples of tests/test_fold_b2_window_gpu.py's cases, FOLD "
                   "variant, recorded on an MI355X from a library built at that commit",
           "cases": {name: fn() for name, fn in CASES.items()}}
    with open(FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))
