"""GPU: the FOLD generator's head computes what it computed BEFORE its conv2 went over to k-slices (generate_fold.hip:
wave w forms the partial sums of inputs 32 w .. 32 w + 31 for all 256 outputs, wave 0 adds the eight slices).

One flipped greedy pick diverges a sequence for the rest of a launch, so the yardstick is bit identity: SHA-256 hashes
of ``logits_out``, ``choices_out`` and ``samples``, recorded on an MI355X from a library built at the commit BEFORE the
change (tests/golden/fold_head_logits_sha256.json; its header names that commit).  The FOLD variant is forced, the
weights are make_state_dict(seed=3, gain=2.0, head_gain=6.0), and the history of the teacher-forced cases is random,
because a tiny model's free run settles on one class.  Cases:

* ``tf-q256``: 2 x 2 layers, Q = 256, 3 sequences, 300 steps -- logits and greedy choices;
* ``tf-q64``, ``tf-q128``: the same at Q = 64 and 128 -- padding classes: zero partial sums plus the -inf bias;
* ``tf-multi``: 10 x 3 layers, 17 sequences, 48 steps -- one pipeline serves two sequences, the partial sums' LDS rows
  are reused between the turns;
* ``free-greedy``: 3 sequences, 400 free greedy steps without ``logits_out`` (a head step that writes nothing out), in
  one launch and cut into two at an odd step;
* ``sampled-reference``, ``sampled-model``: T = 1.0 under both sampling rules, ``samples`` and ``logits_out``; and the
  per-sequence launch (mvn_generate_seq) with mixed rows: a greedy one, a truncated one, a sampled one;
* ``guided``: one pair through mvn_generate_guided, two turns per step, 64 steps.

The fixture is only worth something recorded from the parent's library: --record refuses to run unless MOVENET_HIP_LIB
names the library it is to record from, and wants the commit that library was built at.

    MOVENET_HIP_LIB=<library built at that commit> python tests/test_fold_head_slices_gpu.py --record <commit>
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

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fold_head_logits_sha256.json")
DEV = "cuda:0"
C = 64


def _cfg(layer_size, stack_size, Q):
    return dict(layer_size=layer_size, stack_size=stack_size, input_channels=Q, residual_channels=C, skip_channels=C)


@functools.lru_cache(maxsize=None)
def _weights(layer_size, stack_size, Q):
    sd = make_state_dict(**_cfg(layer_size, stack_size, Q), seed=3, gain=2.0, head_gain=6.0)
    return {k: v.to(DEV) for k, v in sd.items()}


def _gen(layer_size, stack_size, Q, batch, n_new, **kw):
    cfg = _cfg(layer_size, stack_size, Q)
    rf = N.check(N.lib().mvn_receptive_fields(N.make_dims(**cfg)), "mvn_receptive_fields")
    g = RingGenerator(**cfg, state_dict=_weights(layer_size, stack_size, Q), batch=batch, n_total=rf + n_new,
                      device=DEV, variant=N.GEN_FOLD, **kw)
    assert g.variant == N.GEN_FOLD and g.rf == rf
    return g


def _settled(g):
    g.check_errors()
    assert int(g.status_word()[0].item()) == 0


def _sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def _teacher_forced(layer_size, stack_size, Q, batch, n_new):
    g = _gen(layer_size, stack_size, Q, batch, n_new, temperature=0.0)
    hist = synthetic_indices(batch, g.n_total, Q, 100 + batch + Q).to(DEV)
    choices, logits = g.teacher_forced(hist, logits_t0=g.rf)
    _settled(g)
    bad = (~torch.isfinite(logits)).nonzero()
    if len(bad):  # (row, step, class) of the first few: recorded with the hashes, so a change of it shows as one
        print(f"Q={Q} B={batch}: {len(bad)} logits are not finite, first at {bad[:4].tolist()}")
    return {"logits": _sha(logits), "choices": _sha(choices[:, g.rf:]), "finite_logits": len(bad) == 0}


def _free_run(g, parts, out, prompt=None):
    """Free run of sum(parts) steps from a prompt of ``prompt`` (default: rf) samples; ``out``: with logits_out /
    choices_out of every step (one launch)."""
    P = prompt or g.rf
    assert P + sum(parts) == g.n_total
    g.prime(synthetic_indices(g.batch, P, g.Q, 4321).to(DEV))
    got = {}
    if out:
        assert len(parts) == 1
        logits = torch.zeros(g.nrows, parts[0], g.Q, dtype=torch.float32, device=DEV)
        choices = torch.full((g.nrows, g.n_total), -1, dtype=torch.int32, device=DEV)
        g._run(g.t, g.n_total - 1, P, logits, choices, P)
        got = {"logits": _sha(logits), "choices": _sha(choices[:, P:])}
    else:
        for n in parts:
            g.advance(n)
    _settled(g)
    got["samples"] = _sha(g.samples_all)
    return got


def _free_greedy():
    one = _free_run(_gen(2, 2, 256, 3, 400, temperature=0.0), (400,), False)
    two = _free_run(_gen(2, 2, 256, 3, 400, temperature=0.0), (201, 199), False)
    assert one == two  # two launches cut at an odd step pick what one launch picks
    return one


def _sampled(rule):
    got = {}
    for k, v in _free_run(_gen(2, 2, 256, 3, 64, temperature=1.0, seed=7, sampling=rule), (64,), True).items():
        got[k] = v
    mixed = dict(temperature=[0.0, 1.0, 0.7], top_k=[0, 40, 0], top_p=[1.0, 0.9, 1.0], seed=[5, 6, 7], rows=[2, 0, 1])
    for k, v in _free_run(_gen(2, 2, 256, 3, 64, sampling=rule, **mixed), (64,), True).items():
        got["seq_" + k] = v
    return got


def _guided():
    vec = torch.randn(1, C, generator=torch.Generator().manual_seed(17)).to(DEV)
    rf = N.check(N.lib().mvn_receptive_fields(N.make_dims(**_cfg(2, 2, 256))), "mvn_receptive_fields")
    g = _gen(2, 2, 256, 1, 65 - rf, temperature=[0.0], top_k=[0], top_p=[1.0], seed=[9], global_context=vec,
             guidance=2.0)
    assert g.nrows == 2 and g.n_total == 65
    return _free_run(g, (64,), True, prompt=1)  # (a one-sample prompt: primed by stepping, both rows of the pair)


CASES = {
    "tf-q256": lambda: _teacher_forced(2, 2, 256, 3, 300),
    "tf-q64": lambda: _teacher_forced(2, 2, 64, 3, 300),
    "tf-q128": lambda: _teacher_forced(2, 2, 128, 3, 300),
    "tf-multi": lambda: _teacher_forced(10, 3, 256, 17, 48),
    "free-greedy": _free_greedy,
    "sampled-reference": lambda: _sampled("reference"),
    "sampled-model": lambda: _sampled("model"),
    "guided": _guided,
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_head_outputs_equal_the_recording(case):
    with open(FIXTURE) as f:
        want = json.load(f)["cases"][case]
    got = CASES[case]()
    print(f"{case}: " + ", ".join(f"{k} {'ok' if got[k] == want.get(k) else 'DIFFERS'}" for k in sorted(got)))
    assert got == want


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record" and os.environ.get("MOVENET_HIP_LIB"), __doc__
    out = {"recorded_from_commit": sys.argv[2],
           "what": "SHA-256 of logits_out / choices_out / samples of tests/test_fold_head_slices_gpu.py's cases, FOLD "
                   "variant, recorded on an MI355X from a library built at that commit",
           "cases": {name: fn() for name, fn in CASES.items()}}
    with open(FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))
