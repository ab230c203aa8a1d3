"""CPU: the host side of the spectral distance -- ``ops.distance_frame_span`` against hand-computed cases
and against a search over every frame, the numpy reference of ``feature_distance`` against closed forms, the new C ABI
entry and its refusals before any launch, and the argument errors of ``python -m movenet_amd.evaluate``."""
import ctypes
import math

import numpy as np
import pytest
import torch

import spectral_reference as R
from movenet_amd import _native as N
from movenet_amd import ops

DB = 10.0 / math.log(10.0)


# ---- distance_frame_span ------------------------------------------------------------------------------------------------
# n_fft = 64 (h = 32), hop = 16, T = 400 (F = 26): frame f covers samples [16 f - 32, 16 f + 32)

def test_span_without_skip():
    # first = ceil(32 / 16) = 2; len 400: last = floor((400 - 64 + 32) / 16) = floor(23) = 23 -> 22 frames
    assert ops.distance_frame_span([400], 400, 64, 16) == ([2], [22])
    # len 250: last = floor(218 / 16) = 13 -> frames 2 .. 13
    assert ops.distance_frame_span([400, 250], 400, 64, 16) == ([2, 2], [22, 12])


def test_span_past_a_prompt():
    # skip = RF = 8: first = ceil(40 / 16) = 3; skip = 16: ceil(48 / 16) = 3 exactly; skip = 17: 4
    assert ops.distance_frame_span([400, 250], 400, 64, 16, skip=8) == ([3, 3], [21, 11])
    assert ops.distance_frame_span([400], 400, 64, 16, skip=16) == ([3], [21])
    assert ops.distance_frame_span([400], 400, 64, 16, skip=17) == ([4], [20])


def test_a_length_shorter_than_one_window_counts_nothing():
    assert ops.distance_frame_span([63, 0, 10], 400, 64, 16) == ([2, 2, 2], [0, 0, 0])
    # one whole window needs frame 2 = samples [0, 64) -- but with skip = 8 the first frame is 3 = [16, 80)
    assert ops.distance_frame_span([64, 79, 80], 400, 64, 16, skip=8) == ([3, 3, 3], [0, 0, 1])
    assert ops.distance_frame_span([64], 400, 64, 16) == ([2], [1])


def test_a_length_on_a_window_edge_both_sides_of_the_floor():
    # frame 13 covers [176, 240): it counts from len 240 on, not at 239; frame 14 = [192, 256) from 256 on
    assert ops.distance_frame_span([239, 240, 241, 255, 256], 400, 64, 16)[1] == [11, 12, 12, 12, 13]


def test_lengths_none_is_every_row_whole():
    assert ops.distance_frame_span(None, 400, 64, 16, skip=8) == ([3], [21])
    assert ops.distance_frame_span(None, 400, 64, 16, skip=8, batch=3) == ([3] * 3, [21] * 3)
    # the smallest window: T = 33, hop = 1, n_fft = 2 -> F = 34, and frame 33 = [32, 34) reaches past the row
    first, count = ops.distance_frame_span(None, 33, 2, 1)
    assert first == [1] and count == [32]      # frames 1 .. 32 cover [0, 2) .. [31, 33)


@pytest.mark.parametrize("T,n_fft,hop,skip", [(400, 64, 16, 0), (400, 64, 16, 8), (333, 32, 7, 5), (50, 64, 16, 0),
                                               (129, 32, 32, 31), (1000, 256, 100, 77)])
def test_span_equals_a_search_over_every_frame(T, n_fft, hop, skip):
    lengths = sorted({0, 1, n_fft - 1, n_fft, n_fft + 1, T // 2, T - 1, T} & set(range(T + 1)))
    assert ops.distance_frame_span(lengths, T, n_fft, hop, skip) == R.distance_frame_span(lengths, T, n_fft, hop, skip)
    first, count = ops.distance_frame_span(np.asarray(lengths), T, n_fft, hop, skip)
    assert all(f + n <= ops.logmel_frames(T, hop) for f, n in zip(first, count))
    assert ops.distance_frame_span(torch.tensor(lengths), T, n_fft, hop, skip) == (first, count)


def test_span_refusals():
    for bad in ([-1], [401], [2.5], [True], "400", 400, [[400]]):
        with pytest.raises(ValueError, match="lengths"):
            ops.distance_frame_span(bad, 400, 64, 16)
    for bad in (-1, 2.5, True, None):
        with pytest.raises(ValueError, match="skip"):
            ops.distance_frame_span([400], 400, 64, 16, skip=bad)
    with pytest.raises(ValueError, match="hop"):
        ops.distance_frame_span([400], 400, 64, 0)


# ---- the numpy reference against closed forms -----------------------------------------------------------------------------

def test_reference_constant_offset_and_identity():
    rng = np.random.default_rng(5)
    b = (rng.integers(-8192, 8193, size=(3, 7, 20)) / 1024.0).astype(np.float32)   # b + c is exact in float32
    c = 0.375
    lsd, l1, pf = R.feature_distance(b + np.float32(c), b, [0, 4, 19], [20, 9, 1])
    assert np.array_equal(l1, [c] * 3)
    assert np.allclose(lsd, c * DB, rtol=1e-15, atol=0)
    assert np.all(pf[1, :4] == 0) and np.all(pf[1, 13:] == 0) and np.allclose(pf[1, 4:13], c * DB, rtol=1e-15)
    lsd, l1, pf = R.feature_distance(b, b)
    assert not lsd.any() and not l1.any() and not pf.any()
    # one frame, two bins, differences 3 and 4: rms = sqrt(12.5), l1 = 3.5
    a = np.zeros((1, 2, 1), np.float32)
    lsd, l1, _ = R.feature_distance(a, a + np.array([3.0, -4.0], np.float32)[None, :, None])
    assert l1[0] == 3.5 and abs(lsd[0] - math.sqrt(12.5) * DB) < 1e-14
    lsd, l1, _ = R.feature_distance(b + 1, b, [3, 3, 3], [0, 0, 0])
    assert not lsd.any() and not l1.any()


# ---- the C ABI -------------------------------------------------------------------------------------------------------------

def test_signatures_hold_the_new_entries_and_the_abi_version_stays():
    assert "mvn_feature_distance" in N.SIGNATURES and "mvn_feature_distance_scratch_floats" in N.SIGNATURES
    lib = N.lib()
    assert hasattr(lib, "mvn_feature_distance") and lib.mvn_abi_version() == 2
    # two doubles per workgroup of 256 frames
    assert lib.mvn_feature_distance_scratch_floats(16, 63) == 4 * 16
    assert lib.mvn_feature_distance_scratch_floats(16, 8192) == 4 * 16 * 32
    assert lib.mvn_feature_distance_scratch_floats(1, 257) == 8
    assert lib.mvn_feature_distance_scratch_floats(0, 10) == 0 and lib.mvn_feature_distance_scratch_floats(3, 0) == 0


def test_host_refusals_return_bad_arg_before_any_launch():
    lib = N.lib()
    buf = (ctypes.c_double * 64)()     # host memory: never dereferenced, every call below returns before a launch
    p = ctypes.addressof(buf)
    good = dict(a=p, b=p, batch=2, n_mels=5, frames=300, first=p, count=p, lsd=p, l1=p, per_frame=None, scratch=p,
                floats=16)

    def call(**kw):
        v = {**good, **kw}
        return lib.mvn_feature_distance(v["a"], v["b"], v["batch"], v["n_mels"], v["frames"], v["first"], v["count"],
                                        v["lsd"], v["l1"], v["per_frame"], v["scratch"], v["floats"], None)
    for bad in (dict(a=None), dict(b=None), dict(first=None), dict(count=None), dict(lsd=None), dict(l1=None),
                dict(scratch=None), dict(batch=0), dict(batch=-1), dict(n_mels=0), dict(frames=0), dict(batch=65536),
                dict(floats=15), dict(scratch=p + 4)):
        assert call(**bad) == N.MVN_ERR_BAD_ARG, bad
        assert "mvn_feature_distance" in N.last_error() and "bad argument" in N.last_error(), bad
    with pytest.raises(ValueError, match="mvn_feature_distance"):
        N.check(call(batch=0), "mvn_feature_distance")


def test_ops_refuses_cpu_tensors_before_touching_the_library(monkeypatch):
    monkeypatch.setattr(N, "lib", lambda: pytest.fail("the library was asked for"))
    a = torch.zeros(2, 5, 9)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.feature_distance(a, a)


# ---- the command line's argument errors -----------------------------------------------------------------------------------

FLAGS = dict(input_channels=64, residual_channels=16, skip_channels=8, layer_size=3, stack_size=2)


@pytest.fixture(scope="module")
def checkpoints(tmp_path_factory):
    from movenet_amd.wavenet import WaveNet
    d = tmp_path_factory.mktemp("ckpt")
    plain = WaveNet(**FLAGS)
    torch.save({"state_dict": {f"model.{k}": v for k, v in plain.state_dict().items()}}, d / "plain.ckpt")
    labelled = WaveNet(**FLAGS, global_classes=2)
    torch.save({"state_dict": {f"model.{k}": v for k, v in labelled.state_dict().items()},
                "global_classes": ["music", "speech"]}, d / "labelled.ckpt")
    return d


def _fails(argv, capsys, match):
    from movenet_amd import evaluate as E
    with pytest.raises(SystemExit) as e:
        E.main(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert match in err, err


def test_evaluate_parser_errors(checkpoints, tmp_path, capsys):
    flags = [s for k, v in FLAGS.items() for s in (f"--{k}", str(v))]
    (tmp_path / "empty").mkdir()

    def argv(name, *more):
        return ["--checkpoint", str(checkpoints / name), "--wavs", str(tmp_path / "empty")] + flags + list(more)
    _fails(argv("plain.ckpt", "--synthesize", "1"), capsys, "--synthesize 1 needs a checkpoint trained with --use_mel 1")
    _fails(argv("labelled.ckpt"), capsys, "['music', 'speech']")
    _fails(argv("labelled.ckpt", "--label", "noise"), capsys, "['music', 'speech']")
    _fails(argv("plain.ckpt", "--label", "music"), capsys, "records no global_classes")
    _fails(argv("plain.ckpt"), capsys, "no *.wav in")
    _fails(argv("plain.ckpt", "--batch", "0"), capsys, "--batch must be at least 1")
    _fails(argv("plain.ckpt", "--residual_channels", "32"), capsys, "does not fit")
    _fails(flags, capsys, "--checkpoint")     # both required


def test_a_file_longer_than_one_row_is_refused_by_name_before_anything_is_uploaded(tmp_path):
    import wav_material as M
    from movenet_amd import evaluate as E
    from movenet_amd import synthesize as S
    path = str(tmp_path / "long.wav")
    M.write_wav(path, M.quantise(M.signal("sines", 8000, 200, 1, 0), 2), 8000)
    with pytest.raises(ValueError, match=r"long\.wav is 400 samples long at 16000 Hz: more than the 399 samples"):
        S.wav_indices(None, 16000, [path], "cpu", max_samples=399)
    assert E.MAX_ROW_SAMPLES == 2 ** 21
