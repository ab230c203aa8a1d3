"""CPU: the host side of top-k / top-p truncation -- the trainer's flags and config fields, the model properties, the
C ABI's binding and argument check, and the float64 reference the GPU tests use; none of it needs a device."""
import ctypes
import json
import math
import pickle

import numpy as np
import pytest

import truncation_reference as TR
from movenet_amd import _native as N
from movenet_amd.config import ModelConfig, TrainingConfig, arg_parser, config_from_args

BAD = [(-1, 1.0), (0, 0.0), (0, -0.1), (0, 1.5), (0, math.nan)]
TRUNC_RES, TRUNC_ARGS = N.SIGNATURES["mvn_generate_trunc"]  # (the binding everything below is about)


def test_flag_defaults_and_parsing():
    a = arg_parser().parse_args([])
    assert (a.generate_top_k, a.generate_top_p) == (0, 1.0)
    a = arg_parser().parse_args(["--generate_top_k", "32", "--generate_top_p", "0.9"])
    assert (a.generate_top_k, a.generate_top_p) == (32, 0.9) and isinstance(a.generate_top_k, int)
    with pytest.raises(SystemExit):
        arg_parser().parse_args(["--generate_top_k", "many"])
    assert (TrainingConfig().generate_top_k, TrainingConfig().generate_top_p) == (0, 1.0)
    # the rule names stay the two that exist
    with pytest.raises(SystemExit):
        arg_parser().parse_args(["--generate_sampling", "nucleus"])


def test_config_from_args_and_json_round_trip():
    base = "--dataset synthetic://clips=4,frames=100 --use_video 0".split()
    c = config_from_args(arg_parser().parse_args(base))
    assert (c.generate_top_k, c.generate_top_p) == (0, 1.0)
    c = config_from_args(arg_parser().parse_args(base + ["--generate_top_k", "8", "--generate_top_p", "0.75"]))
    assert (c.generate_top_k, c.generate_top_p) == (8, 0.75)
    back = TrainingConfig.from_json(c.to_json())
    assert (back.generate_top_k, back.generate_top_p) == (8, 0.75)


def test_json_without_the_fields_loads_with_the_defaults():
    d = json.loads(TrainingConfig(generate_top_k=8, generate_top_p=0.5, batch_size=5).to_json())
    assert d.pop("generate_top_k") == 8 and d.pop("generate_top_p") == 0.5
    back = TrainingConfig.from_json(json.dumps(d))  # what a run before the fields existed wrote
    assert (back.generate_top_k, back.generate_top_p, back.batch_size) == (0, 1.0, 5)


def test_dance2music_hands_the_knobs_to_the_model():
    from movenet_amd.pytorch_lightning_trainer import Dance2Music
    mc = ModelConfig(2, 2, 16, 8, 8)
    kw = dict(model_config=mc, use_video=False)
    m = Dance2Music("synthetic://clips=2,frames=40", TrainingConfig(**kw, generate_sampling="model", generate_top_k=4,
                                                                    generate_top_p=0.9))
    assert (m.model.generate_sampling, m.model.generate_top_k, m.model.generate_top_p) == ("model", 4, 0.9)
    m = Dance2Music("synthetic://clips=2,frames=40", TrainingConfig(**kw))
    assert (m.model.generate_top_k, m.model.generate_top_p) == (0, 1.0)
    with pytest.raises(ValueError, match="top_k"):
        Dance2Music("synthetic://clips=2,frames=40", TrainingConfig(**kw, generate_top_k=-2))
    with pytest.raises(ValueError, match="top_p"):
        Dance2Music("synthetic://clips=2,frames=40", TrainingConfig(**kw, generate_top_p=0.0))


def test_model_properties_validate_and_survive_an_older_pickle():
    from movenet_amd.wavenet import WaveNet
    model = WaveNet(2, 2, 16, 8, 8)
    assert (model.generate_top_k, model.generate_top_p) == (0, 1.0)
    model.generate_top_k, model.generate_top_p = 5, 0.25
    assert (model.generate_top_k, model.generate_top_p) == (5, 0.25)
    model.generate_top_k = 1000  # (>= the class count: the same as off, not an error)
    model.generate_top_p = 1     # (an integer 1 is 1.0)
    assert model.generate_top_k == 1000 and model.generate_top_p == 1.0 and isinstance(model.generate_top_p, float)
    for top_k, top_p in BAD + [(2.0, 1.0), ("8", 1.0), (True, 1.0), (0, "0.9"), (0, None)]:
        with pytest.raises(ValueError, match="top_[kp]"):
            model.generate_top_k, model.generate_top_p = top_k, top_p
    assert model.generate_top_k in (0, 1000) and model.generate_top_p == 1.0  # (a valid k in front of a bad p is set)
    # a module pickled before the attributes existed
    old = pickle.loads(pickle.dumps(model))
    del old._gen_top_k, old._gen_top_p
    assert (old.generate_top_k, old.generate_top_p) == (0, 1.0)
    # generate() keeps the reference's signature
    import inspect
    assert list(inspect.signature(WaveNet.generate).parameters) == ["self", "audio", "video", "global_features",
                                                                    "n_samples", "temperature"]


def test_the_symbol_is_bound():
    name, res, args = "mvn_generate_trunc", TRUNC_RES, TRUNC_ARGS
    ex = N.SIGNATURES["mvn_generate_ex"][1]
    assert res is ctypes.c_int and args == ex[:-1] + [ctypes.c_int, ctypes.c_float, ctypes.c_void_p]
    assert hasattr(N.lib(), name)
    assert N.lib().mvn_abi_version() == 2
    assert N.truncation(0, 1) == (0, 1.0) and N.truncation(7, 0.5) == (7, 0.5)


def test_generate_trunc_refuses_bad_values_before_any_launch():
    lib = N.lib()
    d2 = N.make_dims(10, 3, 256, 64, 64)
    args = (d2, N.GEN_STREAM, None, None, None, 1, 10, 10, 1, 0, 5, 1.0, 0, None, None, 0, None, N.SAMPLE_MODEL)
    for top_k, top_p in BAD:
        assert lib.mvn_generate_trunc(*args, top_k, top_p, None) == N.MVN_ERR_BAD_ARG
        assert "top_k" in N.last_error() and "top_p" in N.last_error()
    # good values get past that check, to the NULL buffers; so does the rule check still come first
    for top_k, top_p in ((0, 1.0), (8, 0.9), (1 << 20, 1e-6)):
        assert lib.mvn_generate_trunc(*args, top_k, top_p, None) == N.MVN_ERR_BAD_ARG
        assert "top_k" not in N.last_error() and "bad argument" in N.last_error()
    assert lib.mvn_generate_trunc(*args[:-1], 2, 8, 0.9, None) == N.MVN_ERR_BAD_ARG
    assert "sampling" in N.last_error()


# ---- the float64 reference itself -------------------------------------------------------------------------------
def test_reference_kept_sets_on_a_hand_example():
    w = np.array([0.05, 0.4, 0.1, 0.2, 0.2, 0.05])  # sums to 1
    k = TR.kept_set
    assert k(w).all() and k(w, 6).all() and k(w, 0, 1.0).all()
    assert k(w, 1).tolist() == [False, True, False, False, False, False]
    assert k(w, 2).tolist() == [False, True, False, True, True, False]            # the tie at the 2nd weight: both kept
    assert k(w, 0, 0.3).tolist() == [False, True, False, False, False, False]     # 0.4 alone reaches 0.3
    assert k(w, 0, 0.5).tolist() == [False, True, False, True, True, False]       # 0.4 < 0.5 <= 0.4 + 0.2 + 0.2
    assert k(w, 0, 0.85).tolist() == [False, True, True, True, True, False]
    assert k(w, 3, 0.6).tolist() == [False, True, False, True, True, False]       # p of S = 0.8: 0.4 < 0.48 <= 0.6
    assert k(w, 3, 0.4).tolist() == [False, True, False, False, False, False]     # 0.32 <= 0.4
    cdf = TR.truncated_cdf(w, k(w, 2))
    assert np.allclose(cdf, [0, 0.5, 0.5, 0.75, 1, 1]) and cdf[-1] == 1.0
    # unclear: an exact tie at the k-th weight is, a clear gap is not
    assert bool(TR.unclear(w, 2)[0]) and not bool(TR.unclear(w, 1)[0]) and not bool(TR.unclear(w, 3)[0])
    # top-p: p S on the edge of a class is unclear, well inside a class is not
    assert bool(TR.unclear(w, 0, 0.4)[1]) and not bool(TR.unclear(w, 0, 0.3)[1])
    assert TR.wide_kept_set(w, 0, 0.4).tolist() == [False, True, False, True, True, False]


def test_reference_always_keeps_the_largest_weight_and_broadcasts():
    rng = np.random.default_rng(5)
    logits = rng.normal(size=(3, 7, 64)) * 5
    for T, top_k, top_p in [(1.0, 8, 1.0), (1.0, 0, 0.9), (0.5, 0, 0.5), (1.0, 40, 0.9), (1.0, 1, 1e-9)]:
        w = TR.model_weights(logits, T)
        kept = TR.kept_set(w, top_k, top_p)
        assert kept.shape == w.shape and np.take_along_axis(kept, w.argmax(-1)[..., None], -1).all()
        assert (kept <= TR.wide_kept_set(w, top_k, top_p)).all()
        if top_k:
            assert (kept.sum(-1) <= top_k).all()  # (no ties in random logits)
        if top_p < 1.0:
            mass = np.where(kept, w, 0).sum(-1) / np.where(TR.kept_set(w, top_k), w, 0).sum(-1)
            assert (mass >= top_p).all()
            smallest = np.where(kept, w, np.inf).min(-1)  # dropping the threshold class must fall short of p S
            assert ((np.where(kept, w, 0).sum(-1) - smallest) / np.where(TR.kept_set(w, top_k), w, 0).sum(-1)
                    < top_p).all()
