"""GPU: the front end by rate (mvn_audio_frontend_var) through the C ABI, on buffers with sentinel bands.

Rows of width 3000 (the kernel's tile is 1024 outputs): clips at 8, 16 and 44.1 kHz, mono and stereo, whose own n_out
is 1, 1024, 1025 and 3000 -- one output, a full tile, one past it, the whole row.  The first n_out entries of a row are
held, bit for bit, to mvn_audio_frontend run on that clip alone with that n_out (which test_audio_frontend_gpu.py pins
against the float64 restatement); behind them: y = 0 and the class mu-law gives 0.0.  Descriptors with n_out = 0,
n_out = width + 1 or a span outside the upload give a row of -1 while the other rows are computed as usual."""
import numpy as np
import pytest
import torch

import wav_material as M
from helpers import _Guard
from movenet_amd import _native as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDTH, Q = 3000, 256
SILENCE = int((Q - 1) / 2.0 + 0.5)
# rate, frames, channels, n_out = round(frames * 16000 / rate)
CLIPS = ((44100, 3, 2, 1), (16000, 1024, 1, 1024), (44100, 2825, 2, 1025), (8000, 1500, 1, WIDTH))


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


@pytest.fixture(scope="module")
def clips():
    out = []
    for seed, (rate, frames, channels, n_out) in enumerate(CLIPS):
        pcm = M.as_pcm16(M.quantise(M.signal("sines", rate, frames, channels, seed), 2))
        out.append(dict(pcm=pcm, frames=frames, channels=channels, n_out=n_out))
    return out


def _alone(clip, normalize):
    """mvn_audio_frontend on one clip with n_out = its own"""
    from movenet_amd.ops import audio_frontend
    pcm = torch.from_numpy(clip["pcm"].reshape(-1)).to(DEV)
    return audio_frontend(pcm, [clip["frames"]], [clip["channels"]], Q, n_out=clip["n_out"], normalize=normalize,
                          return_waveform=True)


def _var(clips, desc, normalize=True):
    B = len(desc)
    lib = N.lib()
    pcm = torch.from_numpy(np.concatenate([c["pcm"].reshape(-1) for c in clips])).to(DEV)
    guard = _Guard(front=True)
    y = guard.new((B, WIDTH), fill=-7.0, name="y")
    idx = guard.new((B, WIDTH), fill=-77, name="index", dtype=torch.int32)
    scratch = guard.new((max(lib.mvn_audio_frontend_var_scratch_floats(B, WIDTH), 2),), fill=float("nan"),
                        name="scratch")
    d = torch.from_numpy(desc).to(DEV)
    rc = lib.mvn_audio_frontend_var(pcm.data_ptr(), pcm.numel(), d.data_ptr(), B, Q, WIDTH, int(normalize),
                                    y.data_ptr(), scratch.data_ptr(), idx.data_ptr(), _stream())
    assert rc == N.MVN_OK, N.last_error()
    guard.check("mvn_audio_frontend_var")
    return idx, y


def _desc(clips, **over):
    from movenet_amd.ops import audio_clip_var_descriptors
    return audio_clip_var_descriptors([c["frames"] for c in clips], [c["channels"] for c in clips],
                                      [c["n_out"] for c in clips], **over)


@pytest.mark.parametrize("normalize", [True, False])
def test_rows_are_the_plain_front_end_of_each_clip_alone(clips, normalize):
    assert N.lib().mvn_audio_frontend_var_scratch_floats(len(clips), WIDTH) == 2 * len(clips) * 3
    idx, y = _var(clips, _desc(clips), normalize)
    again = _var(clips, _desc(clips), normalize)
    assert torch.equal(idx, again[0]) and torch.equal(y.view(torch.int32), again[1].view(torch.int32))
    for b, c in enumerate(clips):
        n = c["n_out"]
        want_i, want_y = _alone(c, normalize)
        assert torch.equal(idx[b, :n], want_i[0]), (b, n)
        assert torch.equal(y[b, :n].view(torch.int32), want_y[0].view(torch.int32)), (b, n)
        assert bool((idx[b, n:] == SILENCE).all()) and bool((y[b, n:].view(torch.int32) == 0).all()), (b, n)
    assert sorted(c["n_out"] for c in clips) == [1, 1024, 1025, WIDTH]


def test_refused_descriptors_mark_their_row_and_leave_the_others(clips):
    good, _ = _var(clips, _desc(clips))
    rec_t = [("offset", "<i8"), ("frames", "<i4"), ("channels", "<i4"), ("n_out", "<i4"), ("reserved", "<i4")]
    total = sum(c["pcm"].size for c in clips)
    for what, field, value in (("n_out = 0", "n_out", 0), ("n_out = width + 1", "n_out", WIDTH + 1),
                               ("span past the upload", "offset", total - 10)):
        desc = _desc(clips)
        desc.view(rec_t).reshape(len(clips))[field][1] = value
        idx, y = _var(clips, desc)
        assert bool((idx[1] == -1).all()) and bool((y[1] == 0).all()), what
        for b in (0, 2, 3):
            assert torch.equal(idx[b], good[b]), (what, b)
    # the host's own refusals, before any launch
    lib = N.lib()
    assert lib.mvn_audio_frontend_var(None, 10, None, 1, Q, WIDTH, 1, None, None, None, None) == N.MVN_ERR_BAD_ARG
    assert "mvn_audio_frontend_var" in N.last_error()
