"""CPU: the host side of training on sequences of their own length -- the new library symbols and what they refuse
before any launch, ops.valid_columns' arithmetic and refusals, the float64 restatement of tests/masked_reference.py held
to torch's own cross_entropy, what WaveNet.forward / score refuse before they touch a device, the by-rate loader's
arithmetic (clip lengths, head truncation, crop clamping) on files of tests/wav_material.py, and the two flags.  None of
it needs one."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import masked_reference as MR
from movenet_amd import _native as N

SMALL = dict(layer_size=2, stack_size=2, input_channels=16, residual_channels=8, skip_channels=8)
NEW = ("mvn_softmax_ce_forward_len", "mvn_softmax_ce_backward_len", "mvn_score_columns_len",
       "mvn_audio_frontend_var", "mvn_audio_frontend_var_scratch_floats")


def test_symbols_exported_and_bound():
    lib = N.lib()
    for name in NEW:
        assert hasattr(lib, name) and name in N.SIGNATURES
        assert getattr(lib, name).argtypes == N.SIGNATURES[name][1]
    assert lib.mvn_abi_version() == 2                      # the ABI grew; its version did not move
    # the _len calls are the calls they extend plus one pointer in front of the stream
    for new, old in (("mvn_softmax_ce_forward_len", "mvn_softmax_ce_forward_ex"),
                     ("mvn_softmax_ce_backward_len", "mvn_softmax_ce_backward_ex"),
                     ("mvn_score_columns_len", "mvn_score_columns")):
        a, b = N.SIGNATURES[new][1], N.SIGNATURES[old][1]
        assert a == b[:-1] + [C.c_void_p] + b[-1:]
    assert lib.mvn_audio_frontend_var_scratch_floats(16, 160000) == lib.mvn_audio_frontend_scratch_floats(16, 160000)
    assert lib.mvn_audio_frontend_var_scratch_floats(3, 3000) == 18
    assert lib.mvn_audio_frontend_var_scratch_floats(0, 3000) == 0


def test_len_calls_refuse_before_any_launch():
    """Non-NULL HOST buffers as dummies: a call that got past the check would hand them to a kernel."""
    lib = N.lib()
    a = C.addressof
    buf, tg, lp, cp, valid = (C.c_float * 64)(), (C.c_longlong * 8)(), (C.c_float * 4)(), (C.c_int32 * 4)(), (C.c_int32 * 1)()
    fwd = lib.mvn_softmax_ce_forward_len
    for args in ((None, a(tg), 1, 8, 8, a(lp), a(cp), 0, a(valid), None),
                 (a(buf), None, 1, 8, 8, a(lp), a(cp), 0, a(valid), None),
                 (a(buf), a(tg), 1, 8, 8, None, a(cp), 1, a(valid), None),
                 (a(buf), a(tg), 1, 8, 8, a(lp), None, 1, a(valid), None),
                 (a(buf), a(tg), 1, 8, 8, a(lp), a(cp), 2, a(valid), None),       # no such rule
                 (a(buf), a(tg), 1, 8, 8, a(lp), a(cp), -1, None, None),
                 (a(buf), a(tg), -1, 8, 8, a(lp), a(cp), 0, a(valid), None),
                 (a(buf), a(tg), 1, 1, 8, a(lp), a(cp), 0, a(valid), None)):
        assert fwd(*args) == N.MVN_ERR_BAD_ARG and "mvn_softmax_ce_forward_len" in N.last_error()
    bwd = lib.mvn_softmax_ce_backward_len
    d = (C.c_float * 64)()
    for args in ((None, a(tg), 1, 8, 8, 1.0, None, a(d), 64, 8, 0, 8, 0, a(valid), None),
                 (a(buf), None, 1, 8, 8, 1.0, None, a(d), 64, 8, 0, 8, 0, a(valid), None),
                 (a(buf), a(tg), 1, 8, 8, 1.0, None, None, 64, 8, 0, 8, 1, a(valid), None),
                 (a(buf), a(tg), 1, 8, 8, 1.0, None, a(d), 64, 8, 0, 8, 7, a(valid), None),   # no such rule
                 (a(buf), a(tg), 1, 8, 8, 1.0, None, a(d), 64, 8, 0, 7, 0, a(valid), None),   # window narrower than S
                 (a(buf), a(tg), 1, 8, 8, 1.0, None, a(d), 64, 8, 1, 8, 0, a(valid), None)):  # window past the row
        assert bwd(*args) == N.MVN_ERR_BAD_ARG and "mvn_softmax_ce_backward_len" in N.last_error()
    score = lib.mvn_score_columns_len
    for args in ((a(buf), a(tg), 1, 8, 8, 0.0, a(lp), None, None, None, None, a(d), 2, a(valid), None),
                 (None, a(tg), 1, 8, 8, 1.0, a(lp), None, None, None, None, a(d), 2, a(valid), None),
                 (a(buf), a(tg), 1, 8, 8, 1.0, a(lp), None, None, None, None, a(d), 1, a(valid), None)):
        assert score(*args) == N.MVN_ERR_BAD_ARG and "mvn_score_columns_len" in N.last_error()
    front = lib.mvn_audio_frontend_var
    pcm, idx = (C.c_int16 * 8)(), (C.c_int32 * 8)()
    for args in ((None, 8, a(d), 1, 16, 8, 1, a(buf), a(lp), a(idx), None),
                 (a(pcm), 8, None, 1, 16, 8, 1, a(buf), a(lp), a(idx), None),
                 (a(pcm), 8, a(d), 1, 16, 0, 1, a(buf), a(lp), a(idx), None),                 # width 0
                 (a(pcm), 8, a(d), 0, 16, 8, 1, a(buf), a(lp), a(idx), None),
                 (a(pcm), 8, a(d), 1, 1, 8, 1, a(buf), a(lp), a(idx), None)):
        assert front(*args) == N.MVN_ERR_BAD_ARG and "mvn_audio_frontend_var" in N.last_error()
    assert all(v == 0 for v in buf) and all(v == 0 for v in d) and all(v == 0 for v in lp) and all(v == 0 for v in idx)
    # empty work is not an error and launches nothing
    assert fwd(a(buf), a(tg), 0, 8, 8, a(lp), a(cp), 0, a(valid), None) == N.MVN_OK
    assert bwd(a(buf), a(tg), 0, 8, 8, 1.0, None, a(d), 64, 8, 0, 8, 0, a(valid), None) == N.MVN_OK


def test_valid_columns_arithmetic_and_refusals():
    from movenet_amd.ops import valid_columns
    T, RF = 50, 7
    S = T - RF
    lengths = [0, RF, RF + 1, T, RF - 1, 30]
    assert valid_columns(lengths, T, RF) == [0, 0, 1, S, 0, 23] == MR.valid_columns(lengths, T, RF)
    assert valid_columns(tuple(lengths), T, RF) == valid_columns(np.array(lengths), T, RF) \
        == valid_columns(torch.tensor(lengths), T, RF) == valid_columns(torch.tensor(lengths, dtype=torch.int32), T, RF)
    assert valid_columns([], T, RF) == [] and valid_columns([5], 5, 7) == [0]       # T < RF: no column at all
    for bad in ([-1, 3], [T + 1], [3.0], [True], 5, "12", [[1, 2]], np.zeros((2, 2), dtype=np.int64),
                torch.tensor([1.0]), torch.tensor([[1]]), torch.tensor([True]), torch.tensor([T + 1]),
                torch.tensor([-2])):
        with pytest.raises(ValueError):
            valid_columns(bad, T, RF)


def test_restatement_equals_torch():
    B, Q, S = 3, 9, 11
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, Q, S, generator=g) * 3.0
    tg = torch.randint(0, Q, (B, S), generator=g)
    valid = [S + 4, 5, -1]                                                         # clamped to [S, 5, 0]
    keep = MR.mask(valid, S)
    assert keep.sum(1).tolist() == [S, 5, 0]
    n = int(keep.sum())
    for rule, inp in (("model", x.double()), ("reference", torch.softmax(x.double(), 1))):
        cols = F.cross_entropy(inp, tg, reduction="none")
        loss, acc = MR.masked_loss(x, tg, valid, rule)
        assert abs(loss - cols[keep].sum().item() / n) < 1e-13
        assert acc == ((torch.softmax(x.double(), 1).argmax(1) == tg) & keep).sum().item() / n
        d = MR.masked_dlogit(x, tg, valid, rule, 1.0 / n)
        assert bool((d[~keep[:, None, :].expand_as(d)] == 0).all()) and bool(d[keep[:, None, :].expand_as(d)].any())
        planted = torch.where(keep[:, None, :], x, torch.full_like(x, float("nan")))
        assert torch.equal(MR.masked_dlogit(planted, tg, valid, rule, 1.0 / n), d)
        assert MR.masked_loss(planted, tg, valid, rule)[0] == loss
    p = torch.softmax(x.double(), 1)
    want = (p - F.one_hot(tg, Q).permute(0, 2, 1)) / n
    assert torch.allclose(MR.masked_dlogit(x, tg, valid, "model", 1.0 / n)[:, :, :5][1], want[1, :, :5], atol=1e-15)
    sc = MR.masked_score(x, tg, valid)
    assert torch.allclose(sc["seq_nll"], torch.where(keep, F.cross_entropy(x.double(), tg, reduction="none"),
                                                     torch.zeros((), dtype=torch.float64)).sum(1), atol=1e-13)
    assert bool((sc["rank"][~keep] == -1).all()) and sc["seq_correct"].tolist()[2] == 0
    assert MR.masked_loss(x, tg, [0, 0, 0], "model") == (0.0, 0.0)


def test_model_refuses_bad_lengths_before_any_device():
    from movenet_amd.wavenet import WaveNet
    m = WaveNet(**SMALL)
    T = m.receptive_fields + 20
    x = F.one_hot(torch.randint(0, 16, (2, T)), 16).permute(0, 2, 1).float()     # CPU tensors: nothing may launch
    video = torch.zeros(2, 1, 64, 64, 1)
    with pytest.raises(ValueError, match="video"):
        m(x, video, return_loss=True, lengths=[T, T])
    with pytest.raises(ValueError, match="video"):
        m.score(x, video, lengths=[T, T])
    with pytest.raises(ValueError, match="return_loss"):
        m(x, lengths=[T, T])
    for bad in ([T], [T, T, T], [T, T + 1], [T, -1], [T, 2.5], torch.tensor([[T, T]])):
        with pytest.raises(ValueError, match="lengths"):
            m(x, return_loss=True, lengths=bad)
        with pytest.raises(ValueError, match="lengths"):
            m.score(x, lengths=bad)
    from movenet_amd.wavenet import ScoreResult
    assert ScoreResult(None, None, None, None).positions is None and len(ScoreResult(1, 2, 3, 4, positions=5)) == 6
    assert ScoreResult(1, 2, 3, 4, positions=5).positions == 5


# ---- the loader by rate (WavFolderLoader(clip_length="native")) and its flags ----------------------------------------
def _tree(root, clips):
    """clips: (name, rate, frames, channels) -> <root>/train/a/<name>.wav"""
    import os
    import wav_material as M
    d = os.path.join(str(root), "train", "a")
    os.makedirs(d, exist_ok=True)
    for seed, (name, rate, frames, channels) in enumerate(clips):
        M.write_wav(os.path.join(d, name + ".wav"), M.quantise(M.signal("sines", rate, frames, channels, seed), 2), rate)
    return str(root)


def test_native_plan_head_truncation_and_crop_clamping(tmp_path, monkeypatch):
    import math
    import movenet_amd.wavenet as W
    from movenet_amd.dataset import WavFolderLoader, get_dataloader
    plan, crop = WavFolderLoader.native_plan, WavFolderLoader.cropped_lengths
    F = 8000
    # n_b = min(frames, round(frames_b * audio_rate / rate_b)); a clip that fits is read whole
    assert plan(1600, 8000, F, 16000) == (1600, 3200)
    assert plan(4000, 16000, F, 16000) == (4000, 4000)
    assert plan(2825, 44100, F, 16000) == (2825, 1025)              # round(1024.94)
    assert plan(3, 44100, F, 16000) == (3, 1)
    assert plan(4000, 8000, F, 16000) == (4000, F)                   # exactly the width
    # one that would come out longer contributes its head: ceil(frames * rate_b / audio_rate) source frames -> frames
    assert plan(30000, 44100, F, 16000) == (math.ceil(F * 44100 / 16000), F) == (22050, F)
    assert plan(4001, 8000, F, 16000) == (4000, F)
    assert plan(30000, 44100, F, 8000) == (30000, 5442)              # another audio_rate
    # the crop window [start, start + n): clamp(len_b - start, 0, n)
    assert crop([3200, 4000, 8000, 0], 0, 200) == [200, 200, 200, 0]
    assert crop([3200, 4000, 8000], 3100, 200) == [100, 200, 200]
    assert crop([3200, 4000, 8000], 3200, 200) == [0, 200, 200]
    assert crop([3200, 4000, 8000], 7800, 200) == [0, 0, 200]
    # on files: the loader's own plans (no device is needed to build it)
    monkeypatch.setattr(W, "MAX_AUDIO_FRAMES", F)
    root = _tree(tmp_path, [("a_8k", 8000, 1600, 1), ("b_16k", 16000, 4000, 2), ("c_44k", 44100, 30000, 2)])
    ld = WavFolderLoader(root, 64, 3, clip_length="native", audio_rate=16000)
    assert ld.native and ld.plans == [(1600, 3200), (4000, 4000), (22050, F)] and ld.frames == F
    assert get_dataloader(root, 64, 3, use_video=False, clip_length="native", audio_rate=8000).plans == [
        (1600, 1600), (4000, 2000), (30000, 5442)]
    old = WavFolderLoader(root, 64, 3)                                # the default: every clip onto the whole width
    assert not old.native and old.plans == [(1600, F), (4000, F), (30000, F)] and old.cache is not ld.cache
    with pytest.raises(ValueError, match="use_video"):
        WavFolderLoader(root, 64, 3, clip_length="native", use_video=True)
    for bad in (dict(clip_length="stretch"), dict(clip_length="native", audio_rate=0),
                dict(clip_length="native", audio_rate=16000.0)):
        with pytest.raises(ValueError):
            WavFolderLoader(root, 64, 3, **bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        next(iter(ld))


def test_batch_carries_lengths_beside_its_five_fields():
    from movenet_amd.dataset import Batch
    b = Batch(1, 2, 3, 4, 5, lengths=[7])
    assert tuple(b) == (1, 2, 3, 4, 5) and b.lengths == [7] and Batch(1, 2, 3, 4, 5).lengths is None


def test_flags_parse_and_round_trip():
    from movenet_amd.config import TrainingConfig, arg_parser, config_from_args
    args = arg_parser().parse_args([])
    assert args.clip_length == "resample" and args.audio_rate == 16000
    assert TrainingConfig().clip_length == "resample" and TrainingConfig().audio_rate == 16000
    base = "--dataset synthetic://clips=4,frames=100 --use_video 0".split()
    c = config_from_args(arg_parser().parse_args(base + ["--clip_length", "native", "--audio_rate", "22050"]))
    assert c.clip_length == "native" and c.audio_rate == 22050
    back = TrainingConfig.from_json(c.to_json())
    assert back.clip_length == "native" and back.audio_rate == 22050
    with pytest.raises(SystemExit):
        arg_parser().parse_args(base + ["--clip_length", "stretch"])
    import json
    d = json.loads(TrainingConfig(clip_length="native", batch_size=5).to_json())
    d.pop("clip_length"), d.pop("audio_rate")
    old = TrainingConfig.from_json(json.dumps(d))                    # what a run before the fields existed wrote
    assert old.clip_length == "resample" and old.audio_rate == 16000 and old.batch_size == 5
