"""CPU: local conditioning on log-mel frames -- the filterbank, the frame-count rule, every host refusal of the three C
calls (nothing is launched: the pointers handed over are host memory no kernel could read), the module's parameters
with and without ``local_channels``, the ValueErrors, the trainer's flags and the checkpoint record."""
import ctypes

import numpy as np
import pytest
import torch

import logmel_reference as R
from movenet_amd import _native as N
from movenet_amd import ops
from movenet_amd.wavenet import WaveNet

CFG = dict(layer_size=2, stack_size=2, input_channels=64, residual_channels=32, skip_channels=32)


# ---- the filterbank and the frame count ------------------------------------------------------------------------------
def test_filterbank_small_case_by_hand():
    """(M, N, rate) = (4, 64, 16000): mel(8000) = 2840.02, the six points lie 568.00 mel apart, the four centres at
    458.7, 1218.1, 2475.2 and 4556.0 Hz = bins 1.83, 4.87, 9.90 and 18.22 of 250 Hz: peaks in bins 2, 5, 10 and 18."""
    fb = ops.mel_filterbank(4, 64, 16000, 0.0, 8000.0)
    assert fb.shape == (4, 33) and fb.dtype == np.float64
    assert (fb >= 0).all() and (fb <= 1).all()
    assert fb.argmax(1).tolist() == [2, 5, 10, 18]
    centres = [458.7, 1218.1, 2475.2, 4556.0]
    edges = [0.0] + centres + [8000.0]
    for m, k in enumerate([2, 5, 10, 18]):   # the peak bin's own value from the triangle's flank it lies on
        f, lo, mid, hi = 250.0 * k, edges[m], edges[m + 1], edges[m + 2]
        want = (f - lo) / (mid - lo) if f <= mid else (hi - f) / (hi - mid)
        assert abs(fb[m, k] - want) < 2e-3, (m, fb[m, k], want)
    assert fb[:, 0].tolist() == [0.0] * 4 and fb[3, 32] < 1e-12   # the outer edges carry no weight (f_max: to rounding)
    np.testing.assert_allclose(fb, R.mel_filterbank(4, 64, 16000, 0.0, 8000.0), rtol=0, atol=1e-12)


@pytest.mark.parametrize("args", [(80, 1024, 16000, 0.0, 8000.0), (20, 256, 22050, 50.0, 7600.0), (3, 64, 8000, 0.0, 4000.0)])
def test_filterbank_matches_the_restatement(args):
    fb = ops.mel_filterbank(*args)
    assert fb.shape == (args[0], args[1] // 2 + 1) and (fb >= 0).all()
    np.testing.assert_allclose(fb, R.mel_filterbank(*args), rtol=0, atol=1e-12)
    assert (fb.max(1) > 0).all()   # no empty band at these settings


def test_filterbank_refusals():
    for bad in ((0, 64, 16000, 0.0, 8000.0), (4, 64, 16000, 100.0, 100.0), (4, 64, 16000, -1.0, 8000.0),
                (4, 64, 16000, 0.0, 9000.0)):
        with pytest.raises(ValueError):
            ops.mel_filterbank(*bad)
    assert ops.mel_filterbank(4, 64, 16000).shape == (4, 33)   # f_max defaults to rate / 2


def test_frame_count_rule():
    lib = N.lib()
    for T, hop, N_ in ((100, 16, 64), (1000, 64, 256), (17, 64, 64), (2048, 256, 1024), (16000, 256, 1024), (64, 64, 64)):
        F = T // hop + 1
        assert ops.logmel_frames(T, hop) == F == R.n_frames(T, hop)
        assert F >= ops.local_frames_needed(T, hop) == (T - 1) // hop + 1   # the front end's frames always suffice
        pad = (F + 31) // 32 * 32
        assert lib.mvn_logmel_scratch_floats(3, T, N_, hop) == 3 * T + 3 * (N_ // 2 + 1) * pad
    assert lib.mvn_logmel_scratch_floats(0, 100, 64, 16) == 0
    assert lib.mvn_logmel_scratch_floats(2, 100, 48, 16) == 0     # not a power of two
    assert lib.mvn_upsample_features_scratch_floats(2, 16, 7) == 2 * 16 * 7
    assert lib.mvn_upsample_features_scratch_floats(0, 16, 7) == 0


# ---- host refusals through the C ABI ---------------------------------------------------------------------------------
_HOST = (ctypes.c_float * 64)()   # 16-byte aligned below; never read: every call here ends before a launch
P = (ctypes.addressof(_HOST) + 15) // 16 * 16


def _frontend(**kw):
    a = dict(index=P, batch=2, T=100, classes=256, n_fft=64, hop=16, n_mels=8, window=P, twiddle=P, fbank=P, floor=1e-5,
             energies=0, mel=P, mel_ld=7, scratch=P, scratch_floats=1 << 40)
    a.update(kw)
    return N.lib().mvn_logmel_frontend(a["index"], a["batch"], a["T"], a["classes"], a["n_fft"], a["hop"], a["n_mels"],
                                       a["window"], a["twiddle"], a["fbank"], a["floor"], a["energies"], a["mel"],
                                       a["mel_ld"], a["scratch"], a["scratch_floats"], None)


@pytest.mark.parametrize("kw", [
    dict(index=None), dict(window=None), dict(twiddle=None), dict(fbank=None), dict(mel=None), dict(scratch=None),
    dict(n_fft=16), dict(n_fft=4096), dict(n_fft=96), dict(n_fft=0), dict(hop=0), dict(hop=65), dict(hop=-3),
    dict(n_mels=0), dict(floor=0.0), dict(floor=-1.0), dict(floor=float("nan")), dict(batch=-1), dict(T=0),
    dict(classes=1), dict(mel_ld=6), dict(scratch_floats=10),
    # sizes beyond what the indices and grids are written for: a row above 2^30, a batch of 2^31 samples or more
    dict(T=(1 << 30) + 1, hop=64, mel_ld=1 << 30), dict(T=2 ** 31 - 1, hop=1, mel_ld=2 ** 31 - 1),
    dict(batch=4, T=1 << 29, hop=64, mel_ld=1 << 29),
])
def test_frontend_refusals(kw):
    assert _frontend(**kw) == N.MVN_ERR_BAD_ARG, kw
    assert "mvn_logmel_frontend" in N.last_error()


def test_frontend_empty_batch_is_ok():
    assert _frontend(batch=0) == N.MVN_OK
    assert _frontend(batch=0, n_fft=48) == N.MVN_ERR_BAD_ARG   # the shape is still checked


def _upsample(backward=False, **kw):
    a = dict(mel=P, mel_ld=7, w=P, bias=P, batch=2, M=5, F=7, C=16, hop=16, T=100, ctx=P, ctx_ld=100, scratch=P,
             scratch_floats=2 * 16 * 7, dw=P, dbias=P, dmel=P, dmel_ld=7)
    a.update(kw)
    lib = N.lib()
    if backward:
        return lib.mvn_upsample_features_backward(a["ctx"], a["ctx_ld"], a["mel"], a["mel_ld"], a["w"], a["batch"],
                                                  a["M"], a["F"], a["C"], a["hop"], a["T"], a["dw"], a["dbias"],
                                                  a["dmel"], a["dmel_ld"], a["scratch"], a["scratch_floats"], None)
    return lib.mvn_upsample_features(a["mel"], a["mel_ld"], a["w"], a["bias"], a["batch"], a["M"], a["F"], a["C"],
                                     a["hop"], a["T"], a["ctx"], a["ctx_ld"], a["scratch"], a["scratch_floats"], None)


_BOTH = [dict(mel=None), dict(w=None), dict(ctx=None), dict(scratch=None), dict(batch=-1), dict(M=0), dict(F=0),
         dict(C=0), dict(hop=0), dict(T=0), dict(F=6), dict(mel_ld=6), dict(ctx_ld=96), dict(scratch_floats=2 * 16 * 7 - 1),
         # beyond the sizes the kernels' indices are written for: hop above 2^24, a row or a frame count above 2^30
         dict(hop=(1 << 24) + 1), dict(hop=2 ** 31 - 1), dict(batch=0, T=(1 << 30) + 4, ctx_ld=(1 << 30) + 4, hop=1 << 24),
         dict(batch=0, F=(1 << 30) + 1, mel_ld=(1 << 30) + 1, dmel_ld=(1 << 30) + 1)]


@pytest.mark.parametrize("kw", _BOTH + [dict(bias=None), dict(ctx_ld=101), dict(ctx_ld=102), dict(ctx=P + 4)])
def test_upsample_forward_refusals(kw):
    assert _upsample(**kw) == N.MVN_ERR_BAD_ARG, kw
    assert "mvn_upsample_features:" in N.last_error()


@pytest.mark.parametrize("kw", _BOTH + [dict(dmel_ld=6)])
def test_upsample_backward_refusals(kw):
    assert _upsample(backward=True, **kw) == N.MVN_ERR_BAD_ARG, kw
    assert "mvn_upsample_features_backward" in N.last_error()


def test_upsample_empty_batch_and_exact_frames():
    assert _upsample(batch=0) == N.MVN_OK and _upsample(backward=True, batch=0) == N.MVN_OK
    # 100 samples at hop 16 need (99 // 16) + 1 = 7 frames; 97 samples at hop 16 need 7 too, 96 + 1 = 97 is the last
    # length 7 frames serve at hop 16 with T - 1 a multiple of hop
    assert _upsample(batch=0, T=97, ctx_ld=100) == N.MVN_OK
    assert _upsample(batch=0, T=113, ctx_ld=116) == N.MVN_ERR_BAD_ARG   # (112 // 16) + 1 = 8 frames


# ---- the module --------------------------------------------------------------------------------------------------------
def test_default_module_is_unchanged_and_local_conv_comes_last():
    torch.manual_seed(11)
    plain = WaveNet(**CFG)
    torch.manual_seed(11)
    explicit = WaveNet(**CFG, local_channels=0, local_hop=0)
    torch.manual_seed(11)
    local = WaveNet(**CFG, global_classes=3, local_channels=5, local_hop=16)
    torch.manual_seed(11)
    labelled = WaveNet(**CFG, global_classes=3)
    assert list(plain.state_dict()) == list(explicit.state_dict())
    assert not any(k.startswith("local_conv") for k in plain.state_dict())
    for k, v in plain.state_dict().items():
        assert torch.equal(v, explicit.state_dict()[k]), k
    keys = list(local.state_dict())
    assert keys[-2:] == ["local_conv.weight", "local_conv.bias"] and keys[:-2] == list(labelled.state_dict())
    assert keys[-3] == "global_embedding.weight"
    for k, v in labelled.state_dict().items():   # every other parameter keeps its draw
        assert torch.equal(v, local.state_dict()[k]), k
    assert tuple(local.local_conv.weight.shape) == (32, 5, 1) and tuple(local.local_conv.bias.shape) == (32,)
    assert (local.local_channels, local.local_hop) == (5, 16) and (plain.local_channels, plain.local_hop) == (0, 0)
    assert not any(k.startswith("local_conv") for k in local._decoder_state())


def test_constructor_refusals():
    for kw in (dict(local_channels=5), dict(local_hop=16), dict(local_channels=-1, local_hop=16),
               dict(local_channels=2.0, local_hop=16), dict(local_channels=True, local_hop=1)):
        with pytest.raises(ValueError):
            WaveNet(**CFG, **kw)


def test_local_features_value_errors_before_any_launch():
    """All on CPU tensors: each refusal comes before the first thing that would need the GPU."""
    plain, local = WaveNet(**CFG), WaveNet(**CFG, local_channels=5, local_hop=16)
    rf = local.receptive_fields
    T = rf + 40
    x = torch.zeros(2, 64, T)
    x[:, 0] = 1.0
    feats = torch.zeros(2, 5, (T - 1) // 16 + 1)
    video = torch.zeros(2, 1, 64, 64, 1)

    def generate_of(model):
        """generate() keeps the reference's signature: its frames are the model's ``generate_local_features``."""
        def call(audio, video=None, local_features=None, **kw):
            model.generate_local_features = local_features
            return model.generate(audio, video, **kw)
        return call
    for call in (plain.forward, plain.score, generate_of(plain), WaveNet(**CFG, global_classes=2).classify):
        with pytest.raises(ValueError, match="without local_channels"):
            call(x, local_features=feats)
    for call in (local.forward, local.score, generate_of(local)):
        with pytest.raises(ValueError, match="local_features is required"):
            call(x)
        with pytest.raises(ValueError, match="cannot be combined with video"):
            call(x, video, local_features=feats)
        with pytest.raises(ValueError, match="frames"):   # one frame short
            call(x, local_features=feats[:, :, :-1])
        with pytest.raises(ValueError, match="local_features must be"):
            call(x, local_features=feats[:1])
        with pytest.raises(ValueError, match="local_features must be"):
            call(x, local_features=torch.zeros(2, 4, 9))
    with pytest.raises(ValueError, match="frames"):   # generate: frames for n_samples, not for the prompt
        generate_of(local)(x, n_samples=T + 200, local_features=feats)
    # one call uses the setting up, a refused call included: stale frames never meet another prompt
    assert local.generate_local_features is None and plain.generate_local_features is None
    local.generate_local_features = feats
    assert local.generate_local_features is feats
    local.generate_local_features = None
    assert local.generate_local_features is None
    with pytest.raises(TypeError):   # the signature itself is the reference's
        local.generate(x, local_features=feats)
    # lengths IS accepted with local_features: the lengths' own checks pass and the next refusal is the missing GPU
    with pytest.raises(RuntimeError):
        local(x, return_loss=True, lengths=[T, T - 3], local_features=feats)
    with pytest.raises(ValueError, match="lengths cannot be combined with video"):
        local(x, video, return_loss=True, lengths=[T, T - 3])
    local.global_path = "bias"   # (no label here: nothing for "bias" to refuse yet)
    labelled = WaveNet(**CFG, global_classes=2, local_channels=5, local_hop=16)
    labelled.global_path = "bias"
    with pytest.raises(ValueError, match="global_path 'bias'"):
        labelled(x, None, torch.tensor([0, 1]), local_features=feats)
    bf = WaveNet(2, 2, 64, 64, 64, local_channels=5, local_hop=16)
    bf.forward_precision = "bf16"
    with pytest.raises(ValueError, match="bf16"):   # needs bf16_context, like a video context
        bf(x, local_features=feats)


# ---- trainer flags, the trainer's own refusal, the checkpoint record --------------------------------------------------
def test_config_flags_round_trip():
    from movenet_amd.config import TrainingConfig, arg_parser, config_from_args
    d = config_from_args(arg_parser().parse_args(["--dataset", "x"]))
    assert (d.use_mel, d.mel_bins, d.mel_fft, d.mel_hop, d.mel_fmin, d.mel_fmax) == (False, 80, 1024, 256, 0.0, None)
    c = config_from_args(arg_parser().parse_args(
        ["--dataset", "x", "--use_mel", "1", "--mel_bins", "40", "--mel_fft", "512", "--mel_hop", "128", "--mel_fmin",
         "60", "--mel_fmax", "7000", "--use_video", "0"]))
    assert (c.use_mel, c.mel_bins, c.mel_fft, c.mel_hop, c.mel_fmin, c.mel_fmax) == (True, 40, 512, 128, 60.0, 7000.0)
    back = TrainingConfig.from_json(c.to_json())
    assert (back.use_mel, back.mel_bins, back.mel_fft, back.mel_hop, back.mel_fmin, back.mel_fmax) == (
        True, 40, 512, 128, 60.0, 7000.0)
    import json
    old = json.loads(c.to_json())
    for k in ("use_mel", "mel_bins", "mel_fft", "mel_hop", "mel_fmin", "mel_fmax"):
        del old[k]   # a JSON written before the fields existed
    assert TrainingConfig.from_json(json.dumps(old)).use_mel is False


def test_trainer_module_builds_the_model_and_refuses_video():
    from movenet_amd.config import ModelConfig, TrainingConfig
    from movenet_amd.pytorch_lightning_trainer import Dance2Music
    mc = ModelConfig(layer_size=2, stack_size=2, input_channels=64, residual_channels=16, skip_channels=16)
    with pytest.raises(ValueError, match="use_mel"):
        Dance2Music("synthetic://clips=4,frames=400", TrainingConfig(model_config=mc, use_mel=True, use_video=True))
    m = Dance2Music("synthetic://clips=4,frames=400",
                    TrainingConfig(model_config=mc, use_mel=True, use_video=False, mel_bins=8, mel_fft=64, mel_hop=16))
    assert (m.model.local_channels, m.model.local_hop) == (8, 16) and tuple(m.mel_fbank.shape) == (8, 33)
    assert m.local_conditioning == {"local_channels": 8, "local_hop": 16, "mel_fft": 64, "mel_fmin": 0.0,
                                    "mel_fmax": 8000.0, "audio_rate": 16000}
    off = Dance2Music("synthetic://clips=4,frames=400", TrainingConfig(model_config=mc, use_video=False))
    assert off.use_mel is False and not hasattr(off.model, "local_conv") and off.mel_features(None) is None


def test_checkpoint_record_rebuilds_the_model(tmp_path):
    from movenet_amd import checkpoint
    src = WaveNet(**CFG, local_channels=5, local_hop=16)
    rec = {"local_channels": 5, "local_hop": 16, "mel_fft": 64, "mel_fmin": 0.0, "mel_fmax": 8000.0, "audio_rate": 16000}
    path = tmp_path / "mel.ckpt"
    torch.save({"epoch": 0, "local_conditioning": rec,
                "state_dict": {f"model.{k}": v for k, v in src.state_dict().items()}}, path)
    assert checkpoint.local_conditioning_of(path) == rec
    plain = WaveNet(**CFG)
    checkpoint.load_into(plain, path)   # strict: local_conv must exist by then
    assert (plain.local_channels, plain.local_hop) == (5, 16) and plain.local_conditioning == rec
    assert list(plain.state_dict()) == list(src.state_dict())
    for k, v in src.state_dict().items():
        assert torch.equal(plain.state_dict()[k], v), k
    # a checkpoint without the record loads as before, and reports none
    old = tmp_path / "plain.ckpt"
    torch.save({"state_dict": {f"model.{k}": v for k, v in WaveNet(**CFG).state_dict().items()}}, old)
    assert checkpoint.local_conditioning_of(old) is None
    fresh = WaveNet(**CFG)
    checkpoint.load_into(fresh, old)
    assert not hasattr(fresh, "local_conv")
