"""Host: the F0 conditioning channels where no GPU is needed -- the float64 reference on closed forms, every
refusal of mvn_pitch_features before any launch, the header-derived binding, the ``--mel_f0`` flags and their errors,
the checkpoint record's round trip (a key only when on), the resume refusal and ``synthesize --pitch_shift``'s."""
import ctypes
import math

import numpy as np
import pytest
import torch

import pitch_features_reference as R
from movenet_amd import _native as N
from movenet_amd import checkpoint, ops
from movenet_amd.config import ModelConfig, TrainingConfig, arg_parser, config_from_args
from movenet_amd.wavenet import WaveNet

SHAPE = dict(layer_size=2, stack_size=2, input_channels=64, residual_channels=16, skip_channels=16)
SPEC = "synthetic://clips=6,frames=600,seed=5"


# ---- the reference on closed forms --------------------------------------------------------------------------------------

def test_reference_one_voiced_frame_is_a_constant_row():
    period = np.zeros((1, 9), dtype=np.float32)
    period[0, 6] = 40.0
    out = R.features(period, 8000.0, 100.0)
    assert np.array_equal(out[0, 0], np.full(9, np.log2(8000.0 / (40.0 * 100.0))))  # = 1.0
    assert np.array_equal(out[0, 1], np.arange(9) == 6)


def test_reference_two_voiced_frames_give_an_exact_linear_ramp():
    k, rate, f_ref = 8, 8000.0, 125.0
    period = np.zeros((1, 2 + k + 3), dtype=np.float32)
    period[0, 2], period[0, 2 + k] = 64.0, 16.0          # lf = 0 and 2, exactly
    out = R.features(period, rate, f_ref)
    want = np.concatenate([[0.0, 0.0], 2.0 * np.arange(k + 1) / k, [2.0, 2.0]])
    assert np.array_equal(out[0, 0], want)                # (held in front of and behind them)
    assert out[0, 1].sum() == 2
    assert np.array_equal(R.interpolated(period)[0], (np.arange(13) > 2) & (np.arange(13) < 10))


def test_reference_all_unvoiced_is_zeros_and_the_reference_period_is_zero():
    bad = np.array([[0.0, -3.0, np.nan, -np.inf, 0.0]], dtype=np.float32)
    out = R.features(bad, 8000.0, 125.0)
    assert np.array_equal(out, np.zeros((1, 2, 5)))
    assert np.array_equal(R.features(bad, 8000.0, 125.0, shift=[0.5])[0, 0], np.full(5, 0.5))
    out = R.features(np.full((1, 3), 8000.0 / 125.0, dtype=np.float32), 8000.0, 125.0)   # period = rate / f_ref
    assert np.array_equal(out[0, 0], np.zeros(3)) and np.array_equal(out[0, 1], np.ones(3))


def test_reference_cases_hold_what_the_gpu_test_needs():
    cases = R.cases()
    C = R.CHUNK
    assert C == ops.PITCH_FEATURES_CHUNK
    assert cases["one_frame"].shape == (2, 1) and cases["two_frames"].shape[1] == 2
    F3 = cases["long_gap"].shape[1]
    assert 2 * C < F3 < 3 * C
    assert list(np.nonzero(R.voiced_of(cases["long_gap"][0]))[0]) == [3, F3 - 200] and F3 - 200 - 3 > C
    v = R.voiced_of(cases["edges_and_wave_boundary"])
    assert [int(np.nonzero(~v[r])[0][-1]) + 1 for r in (3, 4, 5)] == [63, 64, 65]   # gaps that end at 63 / 64 / 65
    v = R.voiced_of(cases["chunk_boundary"])
    assert [int(np.nonzero(~v[r])[0][-1]) + 1 for r in range(6)] == [C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1]
    assert [int(np.nonzero(~v[r])[0][0]) for r in range(6, 12)] == [C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1]
    odd = cases["nan_and_negative"]
    assert np.isnan(odd[0]).sum() == 3 and (odd[0] < 0).sum() == 3 and not R.voiced_of(odd[1:]).any()
    for period in cases.values():   # every kind of frame the tolerance speaks of occurs
        ref = R.features(period)
        assert np.isfinite(ref).all() and np.isfinite(R.tolerance(period, ref)).all()
    assert sum(int(R.interpolated(p).sum()) for p in cases.values()) > 500


# ---- the C ABI ----------------------------------------------------------------------------------------------------------

def test_the_binding_holds_the_entry_and_the_abi_version_stays():
    res, args = N.SIGNATURES["mvn_pitch_features"]
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_void_p,
                    ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_void_p]
    lib = N.lib()
    assert lib.mvn_abi_version() == 2 and hasattr(lib, "mvn_pitch_features")


def test_pitch_features_refusals_return_bad_arg_before_any_launch():
    lib = N.lib()
    buf = (ctypes.c_float * 64)()  # host memory: never dereferenced, every call below returns before a launch
    p = ctypes.addressof(buf)
    good = dict(period=p, batch=2, frames=30, rate=8000.0, f_ref=173.2, shift=None, out=p, row=10 * 32, chan=32)

    def call(**kw):
        v = {**good, **kw}
        return lib.mvn_pitch_features(v["period"], v["batch"], v["frames"], v["rate"], v["f_ref"], v["shift"], v["out"],
                                      v["row"], v["chan"], None)
    inf, nan = float("inf"), float("nan")
    for bad in (dict(period=None), dict(out=None), dict(frames=0), dict(frames=-1), dict(frames=2 ** 30 + 1, chan=2 ** 31),
                dict(batch=65536), dict(batch=-1), dict(rate=0.0), dict(rate=-8000.0), dict(rate=inf), dict(rate=nan),
                dict(f_ref=0.0), dict(f_ref=-1.0), dict(f_ref=inf), dict(f_ref=nan),
                dict(chan=29), dict(chan=0), dict(chan=-32), dict(row=61), dict(row=0), dict(row=-320)):
        assert call(**bad) == N.MVN_ERR_BAD_ARG, bad
        assert "mvn_pitch_features" in N.last_error() and "bad argument" in N.last_error(), bad
    assert call(chan=29) == N.MVN_ERR_BAD_ARG and "overlap" in N.last_error()
    assert call(row=61) == N.MVN_ERR_BAD_ARG and "overlap" in N.last_error()
    assert call(batch=0) == N.MVN_OK                      # nothing to do, nothing launched
    with pytest.raises(ValueError, match="mvn_pitch_features"):
        N.check(call(rate=nan), "mvn_pitch_features")


def test_ops_refuse_before_touching_the_library(monkeypatch):
    monkeypatch.setattr(N, "lib", lambda: pytest.fail("the library was asked for"))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.pitch_features(torch.zeros(2, 9), 8000.0, 173.2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.local_features(torch.zeros(2, 100, dtype=torch.int32), 64, {"local_channels": 8, "mel_fft": 64, "local_hop": 16,
                                                                        "mel_fmin": 0.0, "mel_fmax": 4000.0,
                                                                        "audio_rate": 8000})
    assert ops.f0_reference(60.0, 500.0) == math.sqrt(60.0 * 500.0)
    for bad in ((0.0, 500.0), (500.0, 60.0), (60.0, 60.0), (60.0, float("inf")), (float("nan"), 500.0)):
        with pytest.raises(ValueError, match="f0_min"):
            ops.f0_reference(*bad)
    assert ops._shift_values(None, 3) is None and ops._shift_values(0.0, 3) is None and ops._shift_values([0, 0], 2) is None
    assert ops._shift_values(1, 2) == [1.0, 1.0] and ops._shift_values(torch.tensor([0.5, -1.0]), 2) == [0.5, -1.0]
    for bad in ([1.0], [1.0, float("nan")], float("inf"), "1", [True, 1.0]):
        with pytest.raises(ValueError, match="shift"):
            ops._shift_values(bad, 2)


# ---- the flags and the config -------------------------------------------------------------------------------------------

BASE = ["--dataset", SPEC]
MEL = ["--use_mel", "1", "--use_video", "0"]


def test_flags_defaults_and_round_trip():
    a = arg_parser().parse_args([])
    assert (a.mel_f0, a.f0_min, a.f0_max) == (False, 60.0, 500.0)
    c = TrainingConfig()
    assert (c.mel_f0, c.f0_min, c.f0_max) == (False, 60.0, 500.0)
    assert config_from_args(arg_parser().parse_args(BASE + MEL)).mel_f0 is False
    c = config_from_args(arg_parser().parse_args(BASE + MEL + ["--mel_f0", "1", "--f0_min", "80", "--f0_max", "400"]))
    assert (c.mel_f0, c.f0_min, c.f0_max) == (True, 80.0, 400.0)
    back = TrainingConfig.from_json(c.to_json())
    assert (back.mel_f0, back.f0_min, back.f0_max) == (True, 80.0, 400.0)


def test_parser_errors():
    with pytest.raises(ValueError, match="--mel_f0 1 needs --use_mel 1"):
        config_from_args(arg_parser().parse_args(BASE + ["--mel_f0", "1"]))
    for lo, hi in (("500", "500"), ("600", "500"), ("0", "500"), ("-60", "500")):
        with pytest.raises(ValueError, match="0 < f0_min < f0_max"):
            config_from_args(arg_parser().parse_args(BASE + MEL + ["--mel_f0", "1", "--f0_min", lo, "--f0_max", hi]))
    # (off: the range is not looked at)
    assert config_from_args(arg_parser().parse_args(BASE + MEL + ["--f0_min", "600"])).mel_f0 is False
    from movenet_amd.pytorch_lightning_trainer import Dance2Music
    with pytest.raises(ValueError, match="--mel_f0 1 needs --use_mel 1"):
        Dance2Music(SPEC, TrainingConfig(model_config=ModelConfig(**SHAPE), use_video=False, mel_f0=True))
    with pytest.raises(ValueError, match="cannot be combined with --use_video 1"):   # (the refusal that was there)
        Dance2Music(SPEC, TrainingConfig(model_config=ModelConfig(**SHAPE), use_video=True, use_mel=True, mel_f0=True))


# ---- the record, the checkpoint and resuming ----------------------------------------------------------------------------

def _module(tmp_path, **over):
    from movenet_amd.pytorch_lightning_trainer import Dance2Music
    kw = dict(model_config=ModelConfig(**SHAPE), batch_size=2, val_batch_size=2, n_epochs=2, use_video=False,
              use_mel=True, mel_bins=8, mel_fft=64, mel_hop=16, optimizer="AdamW", scheduler=None,
              model_output_path=tmp_path / "run")
    return Dance2Music(SPEC, TrainingConfig(**{**kw, **over}))


def _written(tmp_path, module, name):
    """A checkpoint of one CPU step of ``module``, through the writer the trainer uses."""
    opt = module.configure_optimizers()["optimizer"]
    for p in module.model.parameters():
        p.grad = torch.full_like(p, 0.01)
    opt.step()
    obj = checkpoint.training_checkpoint(module, opt, None, epoch=0, global_step=3, next_epoch=1, batches_done=0,
                                         hyper=checkpoint.hyper_parameters(module.config, SPEC), history_len=3)
    checkpoint.write_checkpoint(obj, tmp_path / name)
    return tmp_path / name


def test_the_record_carries_f0_only_when_on_and_readers_rebuild_the_conv(tmp_path):
    plain, f0 = _module(tmp_path), _module(tmp_path, mel_f0=True, f0_min=80.0, f0_max=320.0)
    assert tuple(plain.model.local_conv.weight.shape) == (16, 8, 1) and plain.model.local_channels == 8
    assert tuple(f0.model.local_conv.weight.shape) == (16, 10, 1) and f0.model.local_channels == 10
    assert "f0" not in plain.local_conditioning and "f0" not in plain.model.local_conditioning
    want = {"f_min": 80.0, "f_max": 320.0, "f_ref": 160.0}
    assert f0.local_conditioning["f0"] == want and f0.model.local_conditioning["f0"] == want
    assert f0.local_conditioning["local_channels"] == 8       # the mel bins: what spectral_distance reads
    p0, p1 = _written(tmp_path, plain, "plain.ckpt"), _written(tmp_path, f0, "f0.ckpt")
    rec0, rec1 = checkpoint.local_conditioning_of(p0), checkpoint.local_conditioning_of(p1)
    assert set(rec0) == {"local_channels", "local_hop", "mel_fft", "mel_fmin", "mel_fmax", "audio_rate"}
    assert rec1 == {**rec0, "f0": want}
    assert checkpoint.f0_record_of(rec0) is None and checkpoint.f0_record_of(None) is None
    assert checkpoint.f0_record_of(rec1) == want
    assert checkpoint.local_channels_of(rec0) == 8 and checkpoint.local_channels_of(rec1) == 10
    a, b = WaveNet(**SHAPE), WaveNet(**SHAPE)
    checkpoint.load_into(a, p0)
    checkpoint.load_into(b, p1)
    assert a.local_channels == 8 and b.local_channels == 10 and b.local_conditioning["f0"] == want
    assert torch.equal(b.local_conv.weight, f0.model.local_conv.weight)
    # synthesize / evaluate build the model from the record as well
    from types import SimpleNamespace

    from movenet_amd.synthesize import load_model

    def fail(message):
        raise AssertionError(message)
    for path, channels in ((p0, 8), (p1, 10)):
        args = SimpleNamespace(checkpoint=str(path), ema=0, preemphasis=None, force_preemphasis=0,
                               **{k: None for k in SHAPE})
        model, rec, _ = load_model(args, fail)
        assert model.local_channels == channels and ("f0" in rec) == (channels == 10)


RUNS = [(dict(), dict(mel_f0=True), "['f0'] is absent"), (dict(mel_f0=True), dict(), "['f0'] is present"),
        (dict(mel_f0=True), dict(mel_f0=True, f0_min=70.0), "['f0']['f_min'] is 60.0, but this run has 70.0"),
        (dict(mel_f0=True, f0_max=400.0), dict(mel_f0=True), "['f0']['f_max'] is 400.0, but this run has 500.0")]


@pytest.mark.parametrize("saved,run,text", RUNS)
def test_resume_under_other_f0_settings_is_refused_before_the_gpu(tmp_path, saved, run, text):
    from movenet_amd.pytorch_lightning_trainer import Trainer
    path = _written(tmp_path, _module(tmp_path, **saved), "last.ckpt")
    trainer = Trainer(max_epochs=2, default_root_dir=tmp_path / "run", device="cpu")
    with pytest.raises(ValueError) as e:
        trainer.fit(_module(tmp_path, **run), ckpt_path=path)
    assert str(path) in str(e.value) and "local_conditioning" + text in str(e.value)


def test_pitch_shift_needs_the_f0_record(tmp_path, capsys):
    from movenet_amd import synthesize as S
    assert S.build_parser().parse_args(["--checkpoint", "c", "--out", "o"]).pitch_shift == 0.0
    path = _written(tmp_path, _module(tmp_path), "plain.ckpt")
    (tmp_path / "wavs").mkdir()
    with pytest.raises(SystemExit) as e:
        S.main(["--checkpoint", str(path), "--from_wavs", str(tmp_path / "wavs"), "--out", str(tmp_path / "out"),
                "--pitch_shift", "12", "--device", "cpu"])
    err = capsys.readouterr().err
    assert e.value.code == 2 and "--pitch_shift 12.0 needs a checkpoint trained with --mel_f0 1" in err
