"""CPU: the host side of scoring -- the float64 restatement the GPU tests compare against (tests/score_reference.py)
held to torch's own log_softmax / cross_entropy, its tie rule on hand-made columns, the two library symbols and their
argument checks, the trainer's flag and config field, the sample logger's rows, and what WaveNet.score / classify and
ops.score_logits refuse before they touch a device.  None of it needs one."""
import ctypes as C
import json
import math

import pytest
import torch
import torch.nn.functional as F

import score_reference as SR
from movenet_amd import _native as N
from movenet_amd.config import TrainingConfig, arg_parser, config_from_args

SMALL = dict(layer_size=2, stack_size=2, input_channels=16, residual_channels=8, skip_channels=8)


@pytest.mark.parametrize("Q,S", [(2, 1), (64, 33), (300, 7)])
@pytest.mark.parametrize("T", [0.5, 1.0, 2.0])
def test_restatement_equals_torch(Q, S, T):
    B = 3
    g = torch.Generator().manual_seed(Q + S)
    x = torch.randn(B, Q, S, generator=g) * 4.0          # fp32 logits, as the kernel reads them
    tg = torch.randint(0, Q, (B, S), generator=g)
    got = SR.score(x, tg, T)
    y = x.double() / T
    ls = F.log_softmax(y, 1)
    assert torch.allclose(got["logp"], -F.cross_entropy(y, tg, reduction="none"), rtol=1e-13, atol=1e-13)
    assert torch.allclose(got["logp"], ls.gather(1, tg[:, None])[:, 0], rtol=1e-13, atol=1e-13)
    assert torch.allclose(got["entropy"], -(ls.exp() * ls).sum(1), rtol=1e-13, atol=1e-13)
    assert torch.allclose(got["seq_nll"], F.cross_entropy(y, tg, reduction="none").sum(1), rtol=1e-13, atol=1e-13)
    # no ties in random logits: the rank is the number of larger classes, rank 0 is torch's argmax
    assert torch.equal(got["rank"], (y > y.gather(1, tg[:, None])).sum(1))
    assert torch.equal(got["seq_correct"], (y.argmax(1) == tg).sum(1))
    # targets out of range count as the nearest class
    wild = tg.clone()
    wild[:, 0] = torch.tensor([-3, Q + 5, 0])
    a, b = SR.score(x, wild, T), SR.score(x, wild.clamp(0, Q - 1), T)
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_restatement_tie_rule_and_masked_classes():
    ninf = -math.inf
    #                 column 0        1          2            3              4
    cols = torch.tensor([[1.0, 5.0, 2.0],     # one maximum
                         [5.0, 5.0, 5.0],     # all tied
                         [5.0, 1.0, 5.0],     # the maximum shared by classes 0 and 2
                         [ninf, 0.0, 0.0],    # a masked class, the rest tied
                         [0.0, ninf, 3.0]]).t()[None]  # (1, Q = 3, S = 5)
    def rank(t):
        return SR.score(cols, torch.tensor([t]), 1.0)["rank"][0].tolist()
    assert rank([1, 0, 0, 1, 2]) == [0, 0, 0, 0, 0]        # the first maximum: rank 0
    assert rank([0, 1, 2, 2, 0]) == [2, 1, 1, 1, 1]        # earlier equals count, later ones do not
    assert rank([2, 2, 1, 0, 1]) == [1, 2, 2, 2, 2]        # a masked target ranks behind everything finite
    got = SR.score(cols, torch.tensor([[1, 2, 2, 0, 1]]), 1.0)
    assert got["seq_correct"].tolist() == [1]
    assert got["logp"][0, 3].item() == ninf and got["logp"][0, 4].item() == ninf
    assert bool(torch.isfinite(got["logp"][0, :3]).all()) and bool(torch.isfinite(got["entropy"]).all())
    assert abs(got["entropy"][0, 1].item() - math.log(3.0)) < 1e-15
    assert abs(got["entropy"][0, 3].item() - math.log(2.0)) < 1e-15   # the masked class adds exactly 0
    # the order of y is the order of the logits at any temperature
    assert torch.equal(SR.score(cols, torch.tensor([[0, 1, 2, 2, 0]]), 0.3)["rank"], SR.score(
        cols, torch.tensor([[0, 1, 2, 2, 0]]), 1.0)["rank"])


def test_symbols_exported_and_bound():
    lib = N.lib()
    for name in ("mvn_score_scratch_floats", "mvn_score_columns"):
        assert hasattr(lib, name) and name in N.SIGNATURES
        assert getattr(lib, name).argtypes == N.SIGNATURES[name][1]
    assert N.SIGNATURES["mvn_score_scratch_floats"][0] is C.c_size_t
    assert lib.mvn_abi_version() == 2                      # the ABI grew; its version did not move
    # one float and one int32 slot per 64-column workgroup
    assert lib.mvn_score_scratch_floats(16, 12928) == 2 * 16 * 202
    assert lib.mvn_score_scratch_floats(3, 65) == 12 and lib.mvn_score_scratch_floats(1, 1) == 2
    assert lib.mvn_score_scratch_floats(0, 100) == 0 and lib.mvn_score_scratch_floats(3, 0) == 0
    assert lib.mvn_score_scratch_floats(-1, 5) == 0


def test_score_columns_refuses_before_any_launch():
    """Non-NULL HOST buffers as dummies: a call that got past the check would hand them to a kernel."""
    lib = N.lib()
    buf, tg = (C.c_float * 64)(), (C.c_longlong * 8)()
    logp, seq = (C.c_float * 8)(), (C.c_float * 1)()
    scratch = (C.c_float * 2)()
    a = C.addressof
    for bad in (0.0, -1.0, math.inf, -math.inf, math.nan):
        rc = lib.mvn_score_columns(a(buf), a(tg), 1, 8, 8, bad, a(logp), None, None, a(seq), None, a(scratch), 2, None)
        assert rc == N.MVN_ERR_BAD_ARG and "mvn_score_columns" in N.last_error() and "temperature" in N.last_error()
        with pytest.raises(ValueError, match="temperature"):
            N.check(rc, "mvn_score_columns")
    for args in ((a(buf), a(tg), 1, 8, 8, 1.0, a(logp), None, None, a(seq), None, a(scratch), 1, None),   # short
                 (a(buf), a(tg), 1, 8, 8, 1.0, a(logp), None, None, a(seq), None, None, 2, None),         # no scratch
                 (None, a(tg), 1, 8, 8, 1.0, a(logp), None, None, a(seq), None, a(scratch), 2, None),
                 (a(buf), None, 1, 8, 8, 1.0, a(logp), None, None, a(seq), None, a(scratch), 2, None),
                 (a(buf), a(tg), -1, 8, 8, 1.0, a(logp), None, None, a(seq), None, a(scratch), 2, None),
                 (a(buf), a(tg), 1, 0, 8, 1.0, a(logp), None, None, a(seq), None, a(scratch), 2, None),
                 (a(buf), a(tg), 1, 8, -8, 1.0, a(logp), None, None, a(seq), None, a(scratch), 2, None)):
        assert lib.mvn_score_columns(*args) == N.MVN_ERR_BAD_ARG and "mvn_score_columns" in N.last_error()
    assert all(v == 0 for v in buf) and all(v == 0 for v in logp) and seq[0] == 0 and all(v == 0 for v in scratch)
    # an empty batch is not an error and launches nothing
    assert lib.mvn_score_columns(None, None, 0, 8, 8, 1.0, None, None, None, None, None, None, 0, None) == N.MVN_OK


def test_flag_parses_and_round_trips():
    assert arg_parser().parse_args([]).score_samples is False
    assert arg_parser().parse_args(["--score_samples", "1"]).score_samples is True
    assert arg_parser().parse_args(["--score_samples", "0"]).score_samples is False
    assert TrainingConfig().score_samples is False
    base = "--dataset synthetic://clips=4,frames=100 --use_video 0".split()
    assert config_from_args(arg_parser().parse_args(base)).score_samples is False
    c = config_from_args(arg_parser().parse_args(base + ["--score_samples", "1"]))
    assert c.score_samples is True
    assert TrainingConfig.from_json(c.to_json()).score_samples is True


def test_config_without_the_field_loads_with_the_default():
    d = json.loads(TrainingConfig(score_samples=True, batch_size=5).to_json())
    assert d.pop("score_samples") is True
    back = TrainingConfig.from_json(json.dumps(d))  # what a run before the field existed wrote
    assert back.score_samples is False and back.batch_size == 5


def test_score_logits_refuses_bad_input_before_any_launch():
    from movenet_amd.ops import score_logits, score_temperature
    x, tg = torch.zeros(2, 8, 5), torch.zeros(2, 5, dtype=torch.int64)
    for bad in (0, 0.0, -1.0, math.inf, math.nan, "1", None, True):
        with pytest.raises(ValueError, match="temperature"):
            score_logits(x, tg, temperature=bad)           # (checked first: no device is asked for)
        with pytest.raises(ValueError, match="temperature"):
            score_temperature(bad)
    assert score_temperature(2) == 2.0
    with pytest.raises(RuntimeError, match="MI355X"):
        score_logits(x, tg)                                # CPU tensors are refused, no fallback


def test_score_logits_shape_checks(monkeypatch):
    """Past the device check (stubbed: the tensors live on the CPU), every mismatch is a ValueError before the library
    is asked for anything."""
    from movenet_amd import ops
    monkeypatch.setattr(ops, "_require_gpu", lambda t, what: None)
    monkeypatch.setattr(N, "lib", lambda: pytest.fail("the library was reached"))
    x = torch.zeros(2, 8, 5)
    for bad_x in (torch.zeros(2, 8), torch.zeros(2, 8, 5, dtype=torch.float64), torch.zeros(2, 8, 5, dtype=torch.int32)):
        with pytest.raises(ValueError, match="logits"):
            ops.score_logits(bad_x, torch.zeros(2, 5, dtype=torch.int64))
    for bad_t in (torch.zeros(2, 4, dtype=torch.int64), torch.zeros(3, 5, dtype=torch.int64), torch.zeros(2, 5),
                  torch.zeros(2, 5, dtype=torch.bool), torch.zeros(2, 8, 5, dtype=torch.int64)):
        with pytest.raises(ValueError, match="target"):
            ops.score_logits(x, bad_t)


def _one_hot(B, Q, T):
    x = torch.zeros(B, Q, T)
    x[:, 0] = 1
    return x


def test_score_and_classify_refuse_what_forward_refuses():
    from movenet_amd.wavenet import ScoreResult, WaveNet
    assert ScoreResult._fields == ("logp", "nll", "bits_per_sample", "accuracy", "entropy", "rank")
    m = WaveNet(**SMALL)
    x = _one_hot(2, 16, 20)
    with pytest.raises(RuntimeError, match="MI355X"):
        m.score(x)                                         # CPU tensors: no fallback
    with pytest.raises(ValueError, match="receptive"):
        m.score(_one_hot(2, 16, m.receptive_fields - 1))
    for bad in (0.0, -2.0, math.nan, math.inf):
        with pytest.raises(ValueError, match="temperature"):
            m.score(x, temperature=bad)
    with pytest.raises(ValueError, match="global_classes"):
        m.classify(x)                                      # no labels to tell apart
    m.forward_precision = "bf16"
    with pytest.raises(ValueError, match="bf16"):
        m.score(x)                                         # residual channels other than 64
    # a labelled model: the label is required, and checked, as forward checks it
    g = WaveNet(**SMALL, global_classes=3)
    with pytest.raises(ValueError, match="global_features is required"):
        g.score(x)
    with pytest.raises(ValueError, match="outside"):
        g.score(x, None, torch.tensor([0, 3]))
    g.global_path = "bias"
    with pytest.raises(ValueError, match="bias"):
        g.score(x, torch.zeros(2, 1, 64, 64, 1), torch.tensor([0, 1]))
    g.global_path = "auto"
    for bad in (0, -5, 1.5, True, None):
        with pytest.raises(ValueError, match="logits_budget_bytes"):
            g.classify(x, logits_budget_bytes=bad)
    for bad in (torch.zeros(2), torch.zeros(3, 3), torch.zeros(2, 3, 1)):
        with pytest.raises(ValueError, match="log_prior"):
            g.classify(x, log_prior=bad)
    with pytest.raises(RuntimeError, match="MI355X"):
        g.classify(x)
    # neither call moves the training flag, even when it raises
    g.train()
    with pytest.raises(RuntimeError):
        g.score(x, None, torch.tensor([0, 1]))
    assert g.training


def test_logger_writes_the_scores_only_when_given(tmp_path, monkeypatch):
    from types import SimpleNamespace
    from movenet_amd import callbacks as CB
    monkeypatch.setattr(CB.LogSamplesCallback, "_decode", staticmethod(lambda t, classes: t.to(torch.float64).numpy()))
    trainer = SimpleNamespace(current_epoch=0, rank=0, root=None)
    module = SimpleNamespace(config=SimpleNamespace(model_config=SimpleNamespace(input_channels=64)))
    batch = (torch.zeros(2, 5), None, None, ["a", "b"], None)
    scores = {"bits_per_sample": torch.tensor([1.5, 2.5]), "source_bits_per_sample": torch.tensor([0.25, 0.75])}
    for sub, extra in (("off", {}), ("on", {"sample_scores": scores})):
        cb = CB.LogSamplesCallback(log_every_n_epochs=1, out_dir=str(tmp_path / sub))
        cb.log_samples("validation", trainer, module,
                       {"output": torch.zeros(2, 5), "generated_output": torch.zeros(2, 5), **extra}, batch, 0)
    off = [json.loads(line) for line in open(tmp_path / "off" / "index.jsonl")]
    on = [json.loads(line) for line in open(tmp_path / "on" / "index.jsonl")]
    assert len(off) == len(on) == 2
    assert not any("bits_per_sample" in r or "source_bits_per_sample" in r for r in off)
    assert [(r["bits_per_sample"], r["source_bits_per_sample"]) for r in on] == [(1.5, 0.25), (2.5, 0.75)]
    strip = lambda r: {k: v for k, v in r.items() if k not in ("bits_per_sample", "source_bits_per_sample")}
    assert [strip(r) for r in on] == off                  # nothing else in a row moves
    # a temperature sweep: one generated row per (clip, temperature), clip-major; the source's score per clip
    cb = CB.LogSamplesCallback(log_every_n_epochs=1, out_dir=str(tmp_path / "sweep"), temperature_sweep=[0.5, 1.0])
    swept = {"bits_per_sample": torch.tensor([1.0, 2.0, 3.0, 4.0]), "source_bits_per_sample": torch.tensor([0.25, 0.75])}
    cb.log_samples("validation", trainer, module,
                   {"output": torch.zeros(2, 5), "generated_output": torch.zeros(4, 5), "sample_scores": swept}, batch, 0)
    rows = [json.loads(line) for line in open(tmp_path / "sweep" / "index.jsonl")]
    assert [(r["fp"], r["temperature"], r["bits_per_sample"], r["source_bits_per_sample"]) for r in rows] == [
        ("a", 0.5, 1.0, 0.25), ("a", 1.0, 2.0, 0.25), ("b", 0.5, 3.0, 0.75), ("b", 1.0, 4.0, 0.75)]
