"""GPU: the FOLD generator computes what it computed BEFORE its stages took their inbox wave by wave
(generate_fold.hip: every wave of a layer stage, and of the head, polls the stage's granules itself and reads its
inputs back from a strip of LDS of its own; before, wave 0 polled for all and a barrier stood behind its LDS write).

Only WHERE the 16 or 32 inputs of a lane come from changed, so the yardstick is bit identity: SHA-256 hashes of
``logits_out``, ``choices_out`` and ``samples``, recorded on an MI355X from a library built at the commit BEFORE the
change (tests/golden/fold_wave_inbox_sha256.json; its header names that commit).  The FOLD variant is forced, the
weights are make_state_dict(seed=3, gain=2.0, head_gain=6.0).  Cases (40 steps each unless said otherwise):

* ``config2``: 10 x 3 layers, 2 sequences, greedy -- a free run with every step's logits and choices, and a
  teacher-forced random history (a free run may settle on few classes); the free run's samples equal STREAM's;
* ``two-by-two``: 2 x 2 layers -- a last layer stage with ONE real layer, and stage 0 and the last stage neighbours;
  the same three things, STREAM too;
* ``q64``: 5 x 2 layers at Q = 64 -- the padded head, a last stage with one real layer;
* ``seventeen``: 17 sequences on 16 pipelines -- one pipeline serves two in turn (the MULTI form);
* ``video``: a video-conditioned run of 2 sequences (the context block of the layer stages);
* ``sampled-reference``, ``sampled-model``: T = 1.0 under both sampling rules through the per-sequence launch (own seeds,
  permuted Philox rows, one truncated row);
* ``guided``: two pairs through mvn_generate_guided, two turns per step, 64 steps;
* ``split``: the ``config2`` free run cut into launches of 7 + 33 steps against the unsplit run.

``check_errors()`` is clean after every launch sequence.  No case makes a hand-off time out.

The fixture is only worth something recorded from the parent's library: --record refuses to run unless MOVENET_HIP_LIB
names the library it is to record from, and wants the commit that library was built at.

    MOVENET_HIP_LIB=<library built at that commit> python tests/test_fold_wave_inbox_gpu.py --record <commit>
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

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fold_wave_inbox_sha256.json")
DEV = "cuda:0"
C = 64
STEPS = 40


def _cfg(layer_size, stack_size, Q):
    return dict(layer_size=layer_size, stack_size=stack_size, input_channels=Q, residual_channels=C, skip_channels=C)


@functools.lru_cache(maxsize=None)
def _weights(layer_size, stack_size, Q):
    sd = make_state_dict(**_cfg(layer_size, stack_size, Q), seed=3, gain=2.0, head_gain=6.0)
    return {k: v.to(DEV) for k, v in sd.items()}


def _rf(layer_size, stack_size, Q):
    return N.check(N.lib().mvn_receptive_fields(N.make_dims(**_cfg(layer_size, stack_size, Q))), "mvn_receptive_fields")


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


def _teacher_forced(shape, batch):
    rf = _rf(*shape)
    g = _gen(shape, batch, rf + STEPS)
    hist = synthetic_indices(batch, g.n_total, shape[2], 100 + batch + shape[2]).to(DEV)
    choices, logits = g.teacher_forced(hist, logits_t0=rf)
    _settled(g)
    assert bool(torch.isfinite(logits).all().item())
    return {"tf_logits": _sha(logits), "tf_choices": _sha(choices[:, rf:])}


def _greedy(shape, batch, stream):
    """Free greedy run with every step's outputs + a teacher-forced history; ``stream``: the samples equal STREAM's."""
    rf = _rf(*shape)
    got, samples = _free_run(_gen(shape, batch, rf + STEPS), (STEPS,), True)
    got.update(_teacher_forced(shape, batch))
    if stream:
        _, want = _free_run(_gen(shape, batch, rf + STEPS, variant=N.GEN_STREAM), (STEPS,), False)
        assert torch.equal(samples, want), "FOLD's greedy samples differ from STREAM's"
    return got


def _video():
    shape, B = (10, 3, 256), 2
    rf = _rf(*shape)
    ctx = torch.from_numpy(np.random.default_rng(9).standard_normal((B, C, rf + STEPS)).astype(np.float32)).to(DEV)
    return _free_run(_gen(shape, B, rf + STEPS, context=ctx), (STEPS,), True)[0]


def _sampled(rule):
    shape = (10, 3, 256)
    per_seq = dict(temperature=[1.0, 1.0, 1.0], top_k=[0, 40, 0], top_p=[1.0, 0.9, 1.0], seed=[5, 6, 7], rows=[2, 0, 1])
    return _free_run(_gen(shape, 3, _rf(*shape) + STEPS, sampling=rule, **per_seq), (STEPS,), True)[0]


def _guided():
    shape = (2, 2, 256)
    vec = torch.randn(2, C, generator=torch.Generator().manual_seed(17)).to(DEV)
    g = _gen(shape, 2, 65, temperature=[0.0, 0.0], top_k=[0, 0], top_p=[1.0, 1.0], seed=[9, 10], global_context=vec,
             guidance=2.0)
    assert g.nrows == 4
    return _free_run(g, (64,), True, prompt=1)[0]  # (a one-sample prompt: primed by stepping, both rows of a pair)


def _split():
    shape = (10, 3, 256)
    rf = _rf(*shape)
    one, _ = _free_run(_gen(shape, 2, rf + STEPS), (STEPS,), False)
    two, _ = _free_run(_gen(shape, 2, rf + STEPS), (7, 33), False)
    assert one == two  # launches of 7 + 33 steps pick what one launch of 40 picks
    return one


CASES = {
    "config2": lambda: _greedy((10, 3, 256), 2, True),
    "two-by-two": lambda: _greedy((2, 2, 256), 2, True),
    "q64": lambda: _greedy((5, 2, 64), 2, False),
    "seventeen": lambda: _free_run(_gen((10, 3, 256), 17, _rf(10, 3, 256) + STEPS), (STEPS,), True)[0],
    "video": _video,
    "sampled-reference": lambda: _sampled("reference"),
    "sampled-model": lambda: _sampled("model"),
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


@pytest.mark.gpu
def test_split_run_is_the_config2_run():
    """The fixture itself: the split case's samples are those of ``config2``'s free run (same prompt, same weights)."""
    with open(FIXTURE) as f:
        cases = json.load(f)["cases"]
    assert cases["split"]["samples"] == cases["config2"]["samples"]


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record" and os.environ.get("MOVENET_HIP_LIB"), __doc__
    out = {"recorded_from_commit": sys.argv[2],
           "what": "SHA-256 of logits_out / choices_out / samples of tests/test_fold_wave_inbox_gpu.py's cases, FOLD "
                   "variant, recorded on an MI355X from a library built at that commit",
           "cases": {name: fn() for name, fn in CASES.items()}}
    with open(FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))
