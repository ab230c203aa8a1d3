"""CPU: the host side of the pitch tracker -- the numpy reference on closed-form inputs, the seeds of the
GPU tests' rows against the cap on unsafe frames, ``ops.pitch_lags``, the frame span with n_fft = win + tau_max, every
refusal of the two C ABI entries before any launch, and the argument errors of ``evaluate --pitch`` and
``--score_pitch``."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch

import pitch_reference as R
from movenet_amd import _native as N
from movenet_amd import ops
from movenet_amd.config import TrainingConfig, arg_parser, config_from_args


# ---- the reference on closed forms --------------------------------------------------------------------------------------

def _sine(period, n=1200):
    return np.sin(2 * np.pi * np.arange(n) / period).astype(np.float32)


def test_reference_finds_a_sine_within_the_resolution_argument():
    # the integer minimum lies within 1 of the true period and the refinement within 1/2 of that
    got = R.track(_sine(37.3), 256, 64, 8, 60, 0.15)
    inside = slice(3, 14)  # frames whose 316 samples lie inside the row
    assert got["voiced"][0, inside].all()
    assert np.all(np.abs(got["period"][0, inside] - 37.3) <= 1.5)
    assert np.all(np.abs(got["period"][0, inside] - got["tau"][0, inside]) <= 0.5)


def test_reference_picks_the_first_dip_not_the_octave_below():
    got = R.track(_sine(37.3), 256, 64, 8, 100, 0.15)  # tau_max >= 2 x 37.3: the second dip is in range
    inside = slice(3, 13)
    assert got["voiced"][0, inside].all() and np.all(np.abs(got["period"][0, inside] - 37.3) <= 1.5)
    assert np.all(got["cmnd"][0, inside, 74:76].min(axis=1) < 0.15)  # (the octave's dip is below the threshold too)


def test_reference_constant_frame_is_unvoiced_with_c_of_one():
    got = R.track(np.full(600, 0.25, np.float32), 64, 16, 4, 40, 0.15)
    inside = slice(4, 34)
    assert np.all(got["cmnd"][0, inside] == 1.0) and not got["voiced"][0, inside].any()
    assert np.all(got["period"][0, inside] == 0.0) and np.all(got["aper"][0, inside] == 1.0)
    assert np.all(got["tau"][0, inside] == 4)  # the smallest lag that attains the minimum
    assert np.all(np.isfinite(got["cmnd"]))


def test_reference_white_noise_is_unvoiced():
    x = np.random.default_rng(3).standard_normal(2000).astype(np.float32) * 0.3
    got = R.track(x, 200, 50, 3, 150, 0.15)
    assert not got["voiced"].any() and np.all(got["period"] == 0.0) and np.all(got["aper"] > 0.15)


@pytest.mark.parametrize("setting", R.SETTINGS)
def test_the_gpu_rows_leave_at_most_one_frame_in_twenty_unsafe(setting):
    win, hop, tau_min, tau_max = setting
    x = R.make_rows(tau_min, tau_max)
    ref = R.track(x, win, hop, tau_min, tau_max, R.THRESHOLD)
    safe, _ = R.safe_frames(ref, R.cmnd_tolerance(x, ref["cmnd"], win, hop, tau_max), tau_min, tau_max, R.THRESHOLD)
    unsafe = (~safe).sum(axis=1)
    print("unsafe frames per row", unsafe.tolist(), "of", safe.shape[1])
    assert np.all(unsafe <= 0.05 * safe.shape[1])
    # the tone is voiced, the constant-and-noise row never; the chirp where a frame is short enough to hold its period
    assert ref["voiced"][0].any() and not ref["voiced"][2].any()
    assert ref["voiced"][1].any() == (win < 512) and not ref["voiced"][1].all()


def test_reference_distance_closed_forms():
    a = np.array([[40.0, 0.0, 50.0, 0.0, 80.0, 60.0]], np.float32)
    b = np.array([[40.0 * 2 ** (100 / 1200), 30.0, 0.0, 0.0, 40.0, 60.0]], np.float32)
    rmse, counts = R.distance(a, b, [0], [6])
    assert counts.tolist() == [[3, 2, 1, 6]]  # both: 0, 4, 5; vuv: 1, 2; gross: frame 4 (an octave)
    e0 = 1200 * math.log2(float(b[0, 0]) / 40.0)
    assert abs(rmse[0] - math.sqrt((e0 ** 2 + 1200.0 ** 2 + 0.0) / 3)) < 1e-9
    assert R.distance(a, b, [1], [3])[1].tolist() == [[0, 2, 0, 3]] and R.distance(a, b, [1], [3])[0][0] == 0.0


# ---- host functions -----------------------------------------------------------------------------------------------------

def test_pitch_lags():
    assert ops.pitch_lags(16000, 60, 500) == (32, 267)
    assert ops.pitch_lags(16000, 50, 400) == (40, 320)
    assert ops.pitch_lags(8000, 60.0, 500.0) == (16, 134)
    assert ops.pitch_lags(22050, 70, 441) == (50, 315)
    for bad in ((0, 60, 500), (16000, 0, 500), (16000, 500, 60), (16000, 60, 60), (float("nan"), 60, 500)):
        with pytest.raises(ValueError, match="pitch_lags"):
            ops.pitch_lags(*bad)


@pytest.mark.parametrize("T,win,tau_max,hop,skip", [(2000, 64, 40, 16, 0), (2000, 200, 150, 50, 7), (2000, 512, 300, 128, 4),
                                                    (700, 201, 150, 33, 12)])
def test_frame_span_with_the_pitch_frame_length_names_the_frames_inside_a_clip(T, win, tau_max, hop, skip):
    L = win + tau_max
    lengths = sorted({0, L - 1, L, L + 1, T // 2, T - 1, T})
    first, count = ops.distance_frame_span(lengths, T, L, hop, skip)
    F = R.frames_of(T, hop)
    for n, f0, k in zip(lengths, first, count):
        inside = [j for j in range(F) if j * hop - L // 2 >= skip and j * hop - L // 2 + L <= n]
        assert inside == list(range(f0, f0 + k)) if inside else k == 0, (n, f0, k)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------

def test_signatures_hold_the_new_entries_and_the_abi_version_stays():
    for name in ("mvn_pitch_frames", "mvn_pitch_scratch_floats", "mvn_pitch_distance"):
        assert name in N.SIGNATURES
    assert N.SIGNATURES["mvn_pitch_distance"][1][6] is ctypes.c_double
    lib = N.lib()
    assert lib.mvn_abi_version() == 2
    assert lib.mvn_pitch_scratch_floats(16, 16000, 1024, 267) == 16 * 16000
    for bad in ((0, 100, 64, 40), (-1, 100, 64, 40), (2, 0, 64, 40), (2, 100, 15, 40), (2, 100, 4097, 40),
                (2, 100, 64, 1), (2, 100, 64, 1025), (65536, 100, 64, 40), (3, 2 ** 30, 64, 40)):
        assert lib.mvn_pitch_scratch_floats(*bad) == 0, bad


def test_pitch_frames_refusals_return_bad_arg_before_any_launch():
    lib = N.lib()
    buf = (ctypes.c_float * 64)()  # host memory: never dereferenced, every call below returns before a launch
    p = ctypes.addressof(buf)
    good = dict(index=p, wave=None, batch=2, n=100, classes=64, win=64, hop=16, tau_min=4, tau_max=40, thr=0.15,
                period=p, aper=p, cmnd=None, scratch=p, floats=200)

    def call(**kw):
        v = {**good, **kw}
        return lib.mvn_pitch_frames(v["index"], v["wave"], v["batch"], v["n"], v["classes"], v["win"], v["hop"],
                                    v["tau_min"], v["tau_max"], v["thr"], v["period"], v["aper"], v["cmnd"],
                                    v["scratch"], v["floats"], None)
    for bad in (dict(wave=p), dict(index=None), dict(period=None), dict(aper=None), dict(scratch=None),
                dict(win=15), dict(win=4097), dict(tau_max=1, tau_min=1), dict(tau_max=1025), dict(tau_min=0),
                dict(tau_min=41), dict(hop=0), dict(hop=2 ** 24 + 1), dict(thr=0.0), dict(thr=-0.1), dict(thr=1.5),
                dict(thr=float("nan")), dict(classes=1), dict(batch=-1), dict(batch=65536), dict(n=0),
                dict(n=2 ** 30 + 1, batch=1), dict(n=2 ** 30, batch=2), dict(floats=199)):
        assert call(**bad) == N.MVN_ERR_BAD_ARG, bad
        assert "mvn_pitch_frames" in N.last_error() and "bad argument" in N.last_error(), bad
    assert call(index=None, wave=p, classes=0, floats=199) == N.MVN_ERR_BAD_ARG  # (classes is ignored with wave)
    assert "scratch" in N.last_error()
    assert call(batch=0, floats=0) == N.MVN_OK  # nothing to do, nothing launched
    with pytest.raises(ValueError, match="mvn_pitch_frames"):
        N.check(call(thr=2.0), "mvn_pitch_frames")


def test_pitch_distance_refusals_return_bad_arg_before_any_launch():
    lib = N.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    good = dict(a=p, b=p, batch=2, frames=30, first=p, count=p, ratio=0.2, rmse=p, counts=p)

    def call(**kw):
        v = {**good, **kw}
        return lib.mvn_pitch_distance(v["a"], v["b"], v["batch"], v["frames"], v["first"], v["count"], v["ratio"],
                                      v["rmse"], v["counts"], None)
    for bad in (dict(a=None), dict(b=None), dict(first=None), dict(count=None), dict(rmse=None), dict(counts=None),
                dict(batch=0), dict(batch=-1), dict(batch=65536), dict(frames=0), dict(ratio=0.0), dict(ratio=-1.0),
                dict(ratio=float("inf")), dict(ratio=float("nan"))):
        assert call(**bad) == N.MVN_ERR_BAD_ARG, bad
        assert "mvn_pitch_distance" in N.last_error() and "bad argument" in N.last_error(), bad


def test_ops_refuse_cpu_tensors_and_bad_settings_before_touching_the_library(monkeypatch):
    monkeypatch.setattr(N, "lib", lambda: pytest.fail("the library was asked for"))
    kw = dict(win=64, hop=16, tau_min=4, tau_max=40)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.pitch(torch.zeros(2, 100), **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.pitch_distance(torch.zeros(2, 9), torch.zeros(2, 9))
    for bad in (dict(win=15), dict(win=4097), dict(tau_max=1025), dict(tau_min=0), dict(tau_min=41), dict(hop=0),
                dict(threshold=0.0), dict(threshold=float("nan")), dict(threshold=1.01), dict(win=64.0)):
        with pytest.raises(ValueError):
            ops.check_pitch_settings(**{**kw, "threshold": 0.15, **bad})
    assert ops.check_pitch_settings(64, 16, 4, 40, 1) == (64, 16, 4, 40, 1.0)


# ---- the command line and the config ------------------------------------------------------------------------------------

def test_evaluate_pitch_needs_synthesize(tmp_path, capsys):
    from movenet_amd import evaluate as E
    with pytest.raises(SystemExit) as e:
        E.main(["--checkpoint", str(tmp_path / "none.ckpt"), "--wavs", str(tmp_path), "--pitch", "1"])
    assert e.value.code == 2 and "--pitch 1 needs --synthesize 1" in capsys.readouterr().err
    args = E.build_parser().parse_args(["--checkpoint", "c", "--wavs", "w"])
    assert (args.pitch, args.pitch_fmin, args.pitch_fmax, args.pitch_threshold) == (0, 60.0, 500.0, 0.15)


def test_pitch_summary_pools_over_the_denominators():
    from movenet_amd import evaluate as E
    records = [{"f0_rmse_cents": 30.0, "voiced_frames": 10}, {"f0_rmse_cents": None, "voiced_frames": 0},
               {"f0_rmse_cents": 40.0, "voiced_frames": 30}]
    got = E.pitch_summary(records, [(2, 1, 20), (5, 0, 5), (1, 3, 40)])
    assert got["f0_rmse_cents"] == ((30.0 ** 2 * 10 + 40.0 ** 2 * 30) / 40) ** 0.5
    assert got["vuv_error_rate"] == 8 / 65 and got["gross_pitch_error_rate"] == 4 / 40
    assert E.pitch_summary(records[1:2], [(0, 0, 0)]) == {"f0_rmse_cents": None, "vuv_error_rate": None,
                                                         "gross_pitch_error_rate": None}


BASE = ["--dataset", "synthetic://clips=2,frames=200"]


def test_score_pitch_flag_and_config_round_trip():
    assert arg_parser().parse_args([]).score_pitch is False and TrainingConfig().score_pitch is False
    assert config_from_args(arg_parser().parse_args(BASE)).score_pitch is False
    on = BASE + ["--score_pitch", "1", "--score_samples", "1", "--use_mel", "1", "--use_video", "0"]
    c = config_from_args(arg_parser().parse_args(on))
    assert c.score_pitch is True and TrainingConfig.from_json(c.to_json()).score_pitch is True
    d = json.loads(TrainingConfig(score_pitch=True, score_samples=True, use_mel=True, batch_size=5).to_json())
    assert d.pop("score_pitch") is True  # a JSON written before the field existed
    back = TrainingConfig.from_json(json.dumps(d))
    assert back.score_pitch is False and back.score_samples is True and back.batch_size == 5


def test_score_pitch_needs_score_samples_and_use_mel():
    for flags in (["--score_pitch", "1"], ["--score_pitch", "1", "--score_samples", "1"],
                  ["--score_pitch", "1", "--use_mel", "1", "--use_video", "0"]):
        with pytest.raises(ValueError, match="--score_pitch 1 needs --score_samples 1 --use_mel 1"):
            config_from_args(arg_parser().parse_args(BASE + flags))
    from movenet_amd.config import ModelConfig
    from movenet_amd.pytorch_lightning_trainer import Dance2Music
    mc = ModelConfig(layer_size=2, stack_size=1, input_channels=64, residual_channels=16, skip_channels=16)
    with pytest.raises(ValueError, match="--score_pitch 1 needs"):
        Dance2Music("synthetic://clips=2,frames=200", TrainingConfig(model_config=mc, use_video=False, score_pitch=True,
                                                                    score_samples=True))
