"""CPU: the host side of classifier-free guidance (mvn_gen_guided_max_pairs, the refusals of mvn_generate_guided that
need no device, the config flags, the label-dropout mask, WaveNet.generate_guidance) and the CPU reference's own
sanity (tests/guided_reference.py)."""
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch

import guided_reference as GR
from movenet_amd import _native as N
from movenet_amd.utils.weights import make_state_dict, synthetic_indices
from oracle import wavenet_oracle as O

SMALL = dict(layer_size=2, stack_size=2, input_channels=64, residual_channels=16, skip_channels=16)
CONFIG2 = dict(layer_size=10, stack_size=3, input_channels=256, residual_channels=64, skip_channels=64)
WIDE = dict(layer_size=10, stack_size=6, input_channels=256, residual_channels=128, skip_channels=128)
ANY = 0x3FFFFFFF  # what a one-launch kernel answers: a workgroup per pair


def test_the_two_exports_exist_with_their_signatures():
    """(Fails on a library without the feature: the symbols are missing.)"""
    lib = N.lib()
    assert N.SIGNATURES["mvn_gen_guided_max_pairs"] == (C.c_int, [C.POINTER(N.Dims), C.c_int])
    res, args = N.SIGNATURES["mvn_generate_guided"]
    seq = N.SIGNATURES["mvn_generate_seq"][1]
    # mvn_generate_seq's arguments with the guidance array behind per_seq
    assert res == C.c_int and args == seq[:12] + [C.c_void_p] + seq[12:] and len(args) == 19
    assert lib.mvn_gen_guided_max_pairs.argtypes == [C.POINTER(N.Dims), C.c_int]
    assert lib.mvn_generate_guided.restype == C.c_int
    assert C.sizeof(N.SeqSampling) == 24 and lib.mvn_abi_version() == 2
    header = open(N.__file__.replace("movenet_amd/_native.py", "include/movenet_hip.h")).read()
    assert "int mvn_gen_guided_max_pairs(const mvn_dims *dims, int variant);" in header
    assert "int mvn_generate_guided(" in header


def test_max_pairs():
    lib = N.lib()
    pairs = lambda cfg, v: lib.mvn_gen_guided_max_pairs(N.make_dims(**cfg), v)
    # small dims: GENERIC alone takes them
    assert [pairs(SMALL, v) for v in (N.GEN_GENERIC, N.GEN_STREAM, N.GEN_PIPE, N.GEN_PIPE_F16, N.GEN_FOLD)] == [ANY, 0, 0, 0, 0]
    # config 2: a pipeline per pair -- FOLD's 16 inside the XCDs and 7 across them, PIPE's 24
    assert [pairs(CONFIG2, v) for v in (N.GEN_GENERIC, N.GEN_STREAM, N.GEN_PIPE, N.GEN_PIPE_F16, N.GEN_FOLD)] == [ANY, 0, 24, 0, 23]
    for v in (N.GEN_PIPE, N.GEN_FOLD):
        assert pairs(CONFIG2, v) == lib.mvn_gen_launch_pipelines(N.make_dims(**CONFIG2), v, 1 << 20)
    # C = K = 128, 60 layers: PIPE's 61 stages span two XCDs (4 pipelines), PIPE_F16's 31 fit one each (8)
    assert [pairs(WIDE, v) for v in (N.GEN_GENERIC, N.GEN_STREAM, N.GEN_PIPE, N.GEN_PIPE_F16, N.GEN_FOLD)] == [ANY, 0, 4, 8, 0]
    assert pairs(CONFIG2, 77) == 0
    assert lib.mvn_gen_guided_max_pairs(N.make_dims(0, 3, 256, 64, 64), N.GEN_FOLD) < 0
    assert lib.mvn_gen_guided_max_pairs(None, N.GEN_FOLD) < 0


def _call(variant, pairs, per_seq=1, guidance=1, cfg=CONFIG2):
    """mvn_generate_guided on NULL buffers: only what is refused before any buffer is touched may come back."""
    return N.lib().mvn_generate_guided(N.make_dims(**cfg), variant, None, None, None, pairs, 10, 10, 1, 0, 5,
                                       per_seq or None, guidance or None, None, None, 0, None, N.SAMPLE_MODEL, None)


def test_host_refusals():
    for kw in (dict(per_seq=0), dict(guidance=0), dict(pairs=0), dict(pairs=-3)):
        args = dict(variant=N.GEN_FOLD, pairs=2)
        args.update(kw)
        assert _call(**args) == N.MVN_ERR_BAD_ARG, kw
        assert "mvn_generate_guided" in N.last_error()
    assert _call(N.GEN_STREAM, 1) == N.MVN_ERR_UNSUPPORTED
    assert "STREAM" in N.last_error() and "at most 0 pairs" in N.last_error()
    assert _call(N.GEN_FOLD, 24) == N.MVN_ERR_UNSUPPORTED
    assert "FOLD" in N.last_error() and "at most 23 pairs" in N.last_error() and "24 asked for" in N.last_error()
    assert _call(N.GEN_PIPE, 25) == N.MVN_ERR_UNSUPPORTED and "at most 24 pairs" in N.last_error()
    assert _call(N.GEN_PIPE_F16, 9, cfg=WIDE) == N.MVN_ERR_UNSUPPORTED and "at most 8 pairs" in N.last_error()
    assert _call(N.GEN_FOLD, 1, cfg=SMALL) == N.MVN_ERR_UNSUPPORTED and "at most 0 pairs" in N.last_error()
    # within the limit the call goes on to the ordinary argument check (NULL buffers: bad argument, nothing launched)
    assert _call(N.GEN_GENERIC, 5) == N.MVN_ERR_BAD_ARG and "mvn_generate: bad argument" in N.last_error()
    assert _call(N.GEN_AUTO, 1) == N.MVN_ERR_BAD_ARG


def test_scale_helper():
    assert N.guidance_scales(3, 2) == [2.0, 2.0, 2.0]
    assert N.guidance_scales(3, torch.tensor([0.0, 1.0, -1.5])) == [0.0, 1.0, -1.5]
    assert N.guidance_scales(2, np.array([3.0, 0.5])) == [3.0, 0.5]
    for bad, match in ((math.nan, "row 0"), (math.inf, "row 0"), ([1.0, -math.inf], "row 1"), ([1.0], "1 entries"),
                       ([1.0] * 3, "3 entries"), ("3", "row 0"), (True, "row 0"), (torch.ones(2, 1), "1-D")):
        with pytest.raises(ValueError, match=match):
            N.guidance_scales(2, bad)


def test_config_flags_round_trip_and_old_json_loads():
    from movenet_amd.config import TrainingConfig, arg_parser, config_from_args
    cfg = config_from_args(arg_parser().parse_args(["--dataset", "x"]))
    assert cfg.generate_guidance == 1.0 and cfg.global_dropout == 0.0
    cfg = config_from_args(arg_parser().parse_args(["--dataset", "x", "--generate_guidance", "2.5", "--global_dropout", "0.25"]))
    assert cfg.generate_guidance == 2.5 and cfg.global_dropout == 0.25
    text = cfg.to_json()
    back = TrainingConfig.from_json(text)
    assert back.generate_guidance == 2.5 and back.global_dropout == 0.25
    old = json.loads(text)
    del old["generate_guidance"], old["global_dropout"]
    back = TrainingConfig.from_json(json.dumps(old))
    assert back.generate_guidance == 1.0 and back.global_dropout == 0.0


def _labelled(**kw):
    from movenet_amd.wavenet import WaveNet
    return WaveNet(**SMALL, global_classes=3, **kw)


def test_dropout_mask():
    m = _labelled()
    assert m.global_dropout == 0.0
    m.global_dropout_generator = torch.Generator().manual_seed(5)
    before = m.global_dropout_generator.get_state()
    assert m.global_dropout_mask(8) is None                      # P = 0: the identity ...
    assert torch.equal(m.global_dropout_generator.get_state(), before)  # ... and nothing is drawn
    m.global_dropout = 0.5
    want = torch.Generator().manual_seed(5)
    for _ in range(3):  # the exact rows, step after step
        keep = m.global_dropout_mask(8)
        assert keep.dtype == torch.float32 and torch.equal(keep, (torch.rand(8, generator=want) >= 0.5).float())
    m.global_dropout = 1.0
    assert float(m.global_dropout_mask(8).sum()) == 0.0
    state = torch.random.get_rng_state()
    m.global_dropout_mask(8)
    assert torch.equal(torch.random.get_rng_state(), state)      # torch's own generator is never drawn from
    for bad in (-0.1, 1.5, math.nan, "0.5", True):
        with pytest.raises(ValueError, match="global_dropout"):
            m.global_dropout = bad
    assert sorted(k for k in m.state_dict() if "dropout" in k) == []


def test_generate_guidance_validation():
    from movenet_amd.wavenet import WaveNet
    m = _labelled()
    assert m.generate_guidance == 1.0
    for ok in (3.0, 0, -1.0, [1.0, 2.0], torch.tensor([0.5, 3.0, 1.0])):
        m.generate_guidance = ok
    assert m.generate_guidance == [0.5, 3.0, 1.0]
    for bad in (math.nan, math.inf, [1.0, math.nan], "2", None):
        with pytest.raises((ValueError, TypeError)):
            m.generate_guidance = bad
    assert m.generate_guidance == [0.5, 3.0, 1.0]
    plain = WaveNet(**SMALL)
    plain.generate_guidance = 1.0  # off: any model takes it
    with pytest.raises(ValueError, match="global_classes"):
        plain.generate_guidance = 2.0
    # a wrong length is refused by generate() before anything runs (no device is touched: CPU tensors)
    m.generate_guidance = [1.0, 2.0]
    audio = torch.zeros(3, 64, 40)
    with pytest.raises(ValueError, match="guidance has 2 entries for a batch of 3"):
        m.generate(audio, None, torch.tensor([0, 1, 2]), n_samples=50, temperature=0.0)


def test_logger_records_the_scale(tmp_path, monkeypatch):
    from types import SimpleNamespace
    from movenet_amd import callbacks as CB
    monkeypatch.setattr(CB.LogSamplesCallback, "_decode", staticmethod(lambda t, classes: t.to(torch.float64).numpy()))
    for sub, kw, want in (("off", {}, None), ("one", {"guidance": 1.0}, None), ("on", {"guidance": 2.0}, 2.0)):
        cb = CB.LogSamplesCallback(log_every_n_epochs=1, out_dir=str(tmp_path / sub), **kw)
        trainer = SimpleNamespace(current_epoch=0, rank=0, root=None)
        module = SimpleNamespace(config=SimpleNamespace(model_config=SimpleNamespace(input_channels=64)))
        outputs = {"output": torch.zeros(2, 5), "generated_output": torch.zeros(2, 5)}
        cb.log_samples("validation", trainer, module, outputs, (torch.zeros(2, 5), None, None, ["a", "b"], None), 0)
        rows = [json.loads(line) for line in open(tmp_path / sub / "index.jsonl")]
        assert len(rows) == 2 and all(r.get("guidance") == want for r in rows)


def test_reference_combine_and_scale_one():
    rng = np.random.default_rng(0)
    lc, lu = rng.standard_normal((2, 5, 64)).astype(np.float32), rng.standard_normal((2, 5, 64)).astype(np.float32)
    assert np.array_equal(GR.guided_logits(lc, lu, 1.0).view(np.uint32), lc.view(np.uint32))
    assert np.array_equal(GR.guided_logits(lc, lu, 0.0), lc + np.float32(-1.0) * (lc - lu))
    got = GR.guided_logits(lc, lu, np.array([3.0, -1.0]))
    assert np.array_equal(got[1], lc[1] + np.float32(-2.0) * (lc[1] - lu[1])) and got.dtype == np.float32
    # s = 1 is O.generate_ring with the label's context
    dims = O.Dims(**SMALL)
    sd = make_state_dict(**SMALL, seed=1, gain=1.5, head_gain=6.0)
    rf, n_total, B = dims.receptive_fields, dims.receptive_fields + 24, 2
    prompt = synthetic_indices(B, rf, 64, 7).numpy()
    e = rng.standard_normal((B, 16)).astype(np.float32)
    want, want_logits = O.generate_ring(sd, dims, prompt, n_total, context=np.repeat(e[:, :, None], n_total, 2))
    choices, lu, lc, lg = GR.generate_guided(sd, dims, prompt, n_total, e, 1.0)
    assert np.array_equal(choices, want)
    # (generate_ring hands its steps strided views of a (B, C, T) context, this reference contiguous (B, C) vectors:
    # the BLAS sums the context products in another order, a few ulp of the logits)
    assert np.abs(lc[:, rf:] - want_logits).max() <= 1e-5 * np.abs(want_logits).max()
    assert np.array_equal(lg.view(np.uint32), lc.view(np.uint32)) and not np.array_equal(lu, lc)
