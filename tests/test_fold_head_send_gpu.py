"""GPU: the FOLD generator computes what it computed BEFORE wave 0 of its head read E0's row of the next send a step
ahead (pipe_common.h, head_loop's SEND_AHEAD: the row of the index that becomes idx_prev is read in front of the wait
for the head's input and moves with the index; one sequence per pipeline -- several in turn stay on send_h0).  The
cases also cover what was built with it and not merged (the E1 rows of the four 16-lane rows' candidates
read under the rows' scalar merge, logits_out stored behind the send), which is why they plant the winner's row and
the margin of the clear test.

No operand, product or sum changed, so the yardstick is bit identity: SHA-256 hashes of ``logits_out``, ``choices_out``
and ``samples``, recorded on an MI355X from a library built at the commit BEFORE the change
(tests/golden/fold_head_send_sha256.json; its header names that commit).  The FOLD variant is forced, the weights are
make_state_dict(seed=3, gain=2.0, head_gain=6.0).  Every greedy case is ONE launch from t = 0 (t_begin = 0: there is
no previous sample, idx_prev = -1) over the prompt, 24 teacher-forced steps of a random history and 40 free steps,
unless it says otherwise, and its samples must equal STREAM's as well.

Planted heads.  Which of the four DPP rows of wave 0 (classes 64 r .. 64 r + 63) wins a step, and by what margin,
decides the path a step takes, so the head is planted (tests/planted_logits.py's device: conv2's bias IS the logits):

* ``lean`` planting -- conv2.weight scaled by 2^-10, bias +16 at the winner over a floor of -16: the winner is the
  planted class at every step (asserted), yet every logit still carries the history in its low bits, so a wrong row
  sent at one step shows in the logits of the next.  ``row0`` .. ``row3``: the winner in each 16-lane row in turn
  (classes 21, 85, 149, 213); ``class0``, ``class255``: the first and the last class; ``q64-last``: class 63 of a
  padded Q = 64 head (the candidates of rows 1-3 are padding classes); ``config2-row2``: class 149 at config-2 depth.
* exact planting -- conv2.weight = 0, the logits are the bias bit for bit.  ``tie``: 3.0 at classes 37 and 170 (rows 0
  and 2) over -2.0: the margin is 0, the step takes the full double-softmax form and picks 37; ``under`` / ``over``: the
  runner-up (class 201) 4194 / 4195 ulps of 2^-22 below the winner's 3.0 (class 100) -- margins 0.99993e-3 and
  1.00017e-3 either side of the fp32 1e-3 of the clear test: the nearest pair of fp32 values there is.  (With exact
  planting the logits no longer depend on what was sent; the send of these steps is the fall-back read that the
  teacher-forced and sampled steps of the other cases take too.)

Unplanted: ``two-by-two`` and ``config2`` (10 x 3 layers), ``q64`` (2 x 2 layers, padded head); ``split``: config-2
depth, 40 free steps in launches of 13 + 27 against one launch (the row read ahead crosses a launch boundary at an odd
step); ``seventeen``: 17 sequences on 16 pipelines, 40 free steps (the MULTI form, its indices kept in LDS between
the turns); ``guided``: one pair through mvn_generate_guided (one pair of indices, two puts); ``seq``: a per-sequence
sampled launch (no step leaves through the clear test).

``check_errors()`` is clean after every launch sequence.  No case makes a hand-off time out.

The fixture is only worth something recorded from the parent's library: --record refuses to run unless MOVENET_HIP_LIB
names the library it is to record from, and wants the commit that library was built at.

    MOVENET_HIP_LIB=<library built at that commit> python tests/test_fold_head_send_gpu.py --record <commit>
"""
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from movenet_amd import _native as N
from movenet_amd.generation import RingGenerator
from movenet_amd.utils.weights import make_state_dict, synthetic_indices

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fold_head_send_sha256.json")
DEV = "cuda:0"
C = 64
CONFIG2, TWO_BY_TWO, TWO_BY_TWO_Q64 = (10, 3, 256), (2, 2, 256), (2, 2, 64)
FORCED, FREE = 24, 40
ULP3 = 2.0 ** -22  # one ulp of an fp32 in [2, 4)


def _cfg(layer_size, stack_size, Q):
    return dict(layer_size=layer_size, stack_size=stack_size, input_channels=Q, residual_channels=C, skip_channels=C)


@functools.lru_cache(maxsize=None)
def _weights(shape, plant=None):
    """plant: None, ("lean", winner) or ("exact", ((class, logit), ...), floor)."""
    sd = make_state_dict(**_cfg(*shape), seed=3, gain=2.0, head_gain=6.0)
    if plant is not None:
        Q = shape[2]
        if plant[0] == "lean":
            bias = np.full(Q, -16.0, dtype=np.float32)
            bias[plant[1]] = 16.0
            sd["dense_conv.conv2.weight"] = sd["dense_conv.conv2.weight"] * 2.0 ** -10
        else:
            bias = np.full(Q, plant[2], dtype=np.float32)
            for cls, logit in plant[1]:
                bias[cls] = np.float32(logit)
                assert float(bias[cls]) == logit, "the planted logit is not an fp32 value"
            sd["dense_conv.conv2.weight"] = torch.zeros_like(sd["dense_conv.conv2.weight"])
        assert sd["dense_conv.conv2.bias"].shape == (Q,)
        sd["dense_conv.conv2.bias"] = torch.as_tensor(bias)
    return {k: v.to(DEV) for k, v in sd.items()}


def _rf(shape):
    return N.check(N.lib().mvn_receptive_fields(N.make_dims(**_cfg(*shape))), "mvn_receptive_fields")


def _gen(shape, batch, n_total, variant=N.GEN_FOLD, plant=None, **kw):
    kw.setdefault("temperature", 0.0)
    g = RingGenerator(**_cfg(*shape), state_dict=_weights(shape, plant), batch=batch, n_total=n_total, device=DEV,
                      variant=variant, **kw)
    assert g.variant == variant
    return g


def _settled(g):
    g.check_errors()
    word = g.status_word()
    assert word is None or int(word[0].item()) == 0


def _sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def _forced_then_free(shape, batch, variant=N.GEN_FOLD, plant=None):
    """ONE launch from t = 0: the prompt (rf samples) and FORCED more steps are fed a random history, FREE greedy steps
    follow; logits and choices of the FORCED + FREE steps."""
    rf = _rf(shape)
    g = _gen(shape, batch, rf + FORCED + FREE, variant=variant, plant=plant)
    given = rf + FORCED
    g.reset()
    g.samples_all.zero_()
    g.samples[:, :given] = synthetic_indices(batch, given, shape[2], 100 + batch + shape[2]).to(DEV)
    logits = torch.zeros(g.nrows, FORCED + FREE, g.Q, dtype=torch.float32, device=DEV)
    choices = torch.full((g.nrows, g.n_total), -1, dtype=torch.int32, device=DEV)
    g._run(0, g.n_total - 1, given, logits, choices, rf)
    _settled(g)
    assert bool(torch.isfinite(logits).all().item())
    got = {"logits": _sha(logits), "choices": _sha(choices[:, rf:]), "samples": _sha(g.samples_all)}
    return got, g.samples_all.clone(), choices[:, rf:].clone()


def _greedy(shape, plant=None, winner=None):
    got, samples, choices = _forced_then_free(shape, 2, plant=plant)
    _, want, _ = _forced_then_free(shape, 2, variant=N.GEN_STREAM, plant=plant)
    assert torch.equal(samples, want), "FOLD's greedy samples differ from STREAM's"
    if winner is not None:  # the planted class wins every step, forced ones too (choices_out is the head's own pick)
        assert bool((choices == winner).all().item()), "the planted class did not win every step"
    return got


def _lean(shape, winner):
    return _greedy(shape, ("lean", winner), winner)


def _exact(planted, winner):
    return _greedy(TWO_BY_TWO, ("exact", planted, -2.0), winner)


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


def _split():
    n = _rf(CONFIG2) + FREE
    one, _ = _free_run(_gen(CONFIG2, 2, n), (FREE,), False)
    two, _ = _free_run(_gen(CONFIG2, 2, n), (13, FREE - 13), False)
    assert one == two  # launches of 13 + 27 steps pick what one launch of 40 picks
    return one


def _seventeen():
    n = _rf(CONFIG2) + FREE
    got, samples = _free_run(_gen(CONFIG2, 17, n), (FREE,), True)
    _, want = _free_run(_gen(CONFIG2, 17, n, variant=N.GEN_STREAM), (FREE,), False)
    assert torch.equal(samples, want), "FOLD's greedy samples (two turns on one pipeline) differ from STREAM's"
    return got


def _guided():
    vec = torch.randn(1, C, generator=torch.Generator().manual_seed(17)).to(DEV)
    g = _gen(TWO_BY_TWO, 1, 1 + FREE, temperature=[0.0], top_k=[0], top_p=[1.0], seed=[9], global_context=vec,
             guidance=2.0)
    assert g.nrows == 2
    return _free_run(g, (FREE,), True, prompt=1)[0]  # (a one-sample prompt: primed by stepping, both rows of the pair)


def _seq():
    per_seq = dict(temperature=[1.0, 0.7, 1.0], top_k=[0, 40, 0], top_p=[1.0, 0.9, 1.0], seed=[5, 6, 7], rows=[2, 0, 1])
    return _free_run(_gen(TWO_BY_TWO, 3, _rf(TWO_BY_TWO) + FREE, sampling="model", **per_seq), (FREE,), True)[0]


CASES = {
    "row0": lambda: _lean(TWO_BY_TWO, 21),
    "row1": lambda: _lean(TWO_BY_TWO, 85),
    "row2": lambda: _lean(TWO_BY_TWO, 149),
    "row3": lambda: _lean(TWO_BY_TWO, 213),
    "class0": lambda: _lean(TWO_BY_TWO, 0),
    "class255": lambda: _lean(TWO_BY_TWO, 255),
    "q64-last": lambda: _lean(TWO_BY_TWO_Q64, 63),
    "config2-row2": lambda: _lean(CONFIG2, 149),
    "tie": lambda: _exact(((37, 3.0), (170, 3.0)), 37),
    "under": lambda: _exact(((100, 3.0), (201, 3.0 - 4194 * ULP3)), 100),
    "over": lambda: _exact(((100, 3.0), (201, 3.0 - 4195 * ULP3)), 100),
    "two-by-two": lambda: _greedy(TWO_BY_TWO),
    "config2": lambda: _greedy(CONFIG2),
    "q64": lambda: _greedy(TWO_BY_TWO_Q64),
    "split": _split,
    "seventeen": _seventeen,
    "guided": _guided,
    "seq": _seq,
}


def test_margins_straddle_the_clear_test():
    """The planted margins are the two fp32 values either side of the kernel's fp32 1e-3 (no GPU)."""
    thr = np.float32(1e-3)
    under = np.float32(3.0) - np.float32(3.0 - 4194 * ULP3)
    over = np.float32(3.0) - np.float32(3.0 - 4195 * ULP3)
    assert under < thr <= over and np.float32(over - under) == np.float32(ULP3)


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
           "what": "SHA-256 of logits_out / choices_out / samples of tests/test_fold_head_send_gpu.py's cases, FOLD "
                   "variant, recorded on an MI355X from a library built at that commit",
           "cases": {name: fn() for name, fn in CASES.items()}}
    with open(FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))
