"""GPU: the three front-end entry points compute what they computed BEFORE they shared one row record, one kernel pair
and one launcher (csrc/audio.hip): SHA-256 of every case's ``index`` and ``y`` bytes against a recording made on an
MI355X from a library built at the commit before that change (tests/golden/audio_frontend_sha256.json; its header
names the commit).  The fixture also holds the hashes of every case's PCM and descriptor bytes, so that an input that
drifted is told apart from a kernel that changed.

Inputs are int64 numpy arithmetic only (an index hash folded into int16 plus a triangle wave): no sin, no RNG stream.
The C entry points are called directly on buffers with sentinel bands on both sides, ``y`` and ``index`` pre-filled,
so a write outside them, or a column left unwritten, shows as well.  The kernel's tile is 1024 outputs.

* plain (n_out = 1100, two tiles): a mono and a stereo clip of 3032 frames (near 441 : 160) and a stereo clip of
  22 000 frames -- exactly 20 : 1, where W = 122, an output has 246 taps (more than one block of 128, which this form
  still sums in ONE chain) and a tile is walked in three staged windows of 398 outputs; normalised, un-normalised,
  and at Q = 64;
* by rate (width = 2500): rows of n_out 1, 700 (two whole tiles of silence only), 1025 and 2500, a 20 : 1 row, and a
  refused row (n_out = width + 1) between good rows; normalised and un-normalised;
* windowed (width = 2500): files at 441 : 160 (W = 17) and 20 : 1, each with windows at out_first = 0, in the middle
  and touching the file's end -- taps reach past both edges of the file -- from the TIGHTEST span the call accepts
  (span_first > 0 in the middle); a given (lo, hi) on the middle rows, the window's own range on the others; and a
  refused row (a span one frame short of its taps) between good rows; normalised and un-normalised.

Recording: with MOVENET_AUDIO_FRONTEND_RECORD=<commit> the test writes the fixture instead of comparing.  That is only
worth something from the parent's library, so it refuses to run unless MOVENET_HIP_LIB names the library to record
from (built at <commit>):

    MOVENET_HIP_LIB=<library built at that commit> MOVENET_AUDIO_FRONTEND_RECORD=<commit> \\
        python -m pytest tests/test_audio_frontend_bits_gpu.py
"""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from helpers import _Guard
from movenet_amd import _native as N
from movenet_amd.ops import audio_clip_descriptors, audio_clip_var_descriptors, audio_clip_window_descriptors

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "audio_frontend_sha256.json")
RECORD = os.environ.get("MOVENET_AUDIO_FRONTEND_RECORD")
DEV = "cuda:0"
N_OUT, WIDTH = 1100, 2500


def pcm16(frames: int, channels: int, seed: int) -> np.ndarray:
    """(frames * channels,) int16, interleaved: hashed sample index (+-8192) on a triangle wave (+-8192)"""
    n = np.arange(frames * channels, dtype=np.int64) + 7919 * seed
    v = (n * 1103515245 + 12345) % (1 << 31)
    v = ((v ^ (v >> 13)) * 1664525 + 1013904223) % (1 << 31)
    noise = (v >> 9) % 16384 - 8192
    frame = np.arange(frames * channels, dtype=np.int64) // channels
    tri = np.abs((frame * (37 + seed)) % 4096 - 2048) * 8 - 8192
    return (noise + tri).astype(np.int16)


def tight_span(file_frames: int, orig: int, neu: int, W: int, out_first: int, n_out: int) -> tuple:
    """(span_first, span_frames): the frames of the file the taps of columns [out_first, out_first + n_out) reach"""
    lo = max(0, out_first * orig // neu - W)
    hi = min(file_frames - 1, (out_first + n_out - 1) * orig // neu + W + 1)
    return lo, hi - lo + 1


def plain_inputs():
    clips = [(3032, 1), (3032, 2), (22000, 2)]
    pcm = np.concatenate([pcm16(f, c, s) for s, (f, c) in enumerate(clips)])
    return pcm, audio_clip_descriptors([f for f, _ in clips], [c for _, c in clips])


def var_inputs():
    # frames, channels, n_out: 441 : 160-ish rows, one at 20 : 1, and (third) one whose n_out does not fit the row
    clips = [(3, 2, 1), (1929, 1, 700), (1929, 1, WIDTH + 1), (2825, 2, 1025), (6891, 2, WIDTH), (6000, 1, 300)]
    pcm = np.concatenate([pcm16(f, c, 10 + s) for s, (f, c, _) in enumerate(clips)])
    return pcm, audio_clip_var_descriptors([f for f, _, _ in clips], [c for _, c, _ in clips],
                                           [n for _, _, n in clips])


def window_inputs():
    spans, rows = [], []
    # file_frames, channels, rate_in, (orig, new, W), n_file = ceil(file_frames new / orig)
    for seed, (file_frames, ch, rate_in, (orig, neu, W)) in enumerate(((30000, 2, 44100, (441, 160, 17)),
                                                                        (60000, 1, 320000, (20, 1, 122)))):
        file = pcm16(file_frames, ch, 20 + seed).reshape(file_frames, ch)
        n_file = -(-file_frames * neu // orig)
        # out_first, n_out, (lo, hi), frames the span is short of its taps
        for out_first, n_out, rng, short in ((0, WIDTH if seed == 0 else 700, (0.0, 0.0), 0),
                                             (n_file // 3, 1025, (-0.25, 0.5), 0),
                                             (n_file // 3, 1025, (0.0, 0.0), 1),
                                             (n_file - (700 if seed == 0 else WIDTH), 700 if seed == 0 else WIDTH,
                                              (0.0, 0.0), 0)):
            first, frames = tight_span(file_frames, orig, neu, W, out_first, n_out)
            frames -= short
            spans.append(file[first:first + frames].reshape(-1))
            rows.append((first, frames, file_frames, ch, out_first, n_out, rate_in, rng))
    desc = audio_clip_window_descriptors(*(list(col) for col in zip(*[r[:7] for r in rows])), 16000,
                                         lo=[r[7][0] for r in rows], hi=[r[7][1] for r in rows])
    return np.concatenate(spans), desc


# case -> (inputs, entry point, its row width, Q, normalize)
CASES = {
    "plain-norm": (plain_inputs, "mvn_audio_frontend", N_OUT, 256, 1),
    "plain-raw": (plain_inputs, "mvn_audio_frontend", N_OUT, 256, 0),
    "plain-q64": (plain_inputs, "mvn_audio_frontend", N_OUT, 64, 1),
    "var-norm": (var_inputs, "mvn_audio_frontend_var", WIDTH, 256, 1),
    "var-raw": (var_inputs, "mvn_audio_frontend_var", WIDTH, 256, 0),
    "window-norm": (window_inputs, "mvn_audio_frontend_window", WIDTH, 256, 1),
    "window-raw": (window_inputs, "mvn_audio_frontend_window", WIDTH, 256, 0),
}
REFUSED = {"plain": [], "var": [2], "window": [2, 6]}


def _sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def _inputs(make):
    return make()


def run_case(case: str) -> dict:
    make, entry, width, Q, normalize = CASES[case]
    pcm, desc = _inputs(make)
    B, lib = len(desc), N.lib()
    d_pcm, d_desc = torch.from_numpy(pcm).to(DEV), torch.from_numpy(desc).to(DEV)
    guard = _Guard(front=True)
    y = guard.new((B, width), fill=-7.0, name="y")
    idx = guard.new((B, width), fill=-77, name="index", dtype=torch.int32)
    scratch = guard.new((max(getattr(lib, entry + "_scratch_floats")(B, width), 2),), fill=float("nan"),
                        name="scratch")
    rc = getattr(lib, entry)(d_pcm.data_ptr(), d_pcm.numel(), d_desc.data_ptr(), B, Q, width, normalize, y.data_ptr(),
                             scratch.data_ptr(), idx.data_ptr(), torch.cuda.current_stream(DEV).cuda_stream)
    assert rc == N.MVN_OK, N.last_error()
    guard.check(entry)
    refused = sorted(set(torch.nonzero((idx == -1).all(dim=1)).flatten().tolist()))
    assert refused == REFUSED[case.split("-")[0]], (case, refused)  # (the other rows were formed: the cases reach them)
    assert int(idx.min()) >= -1 and int(idx.max()) < Q
    return dict(pcm=_sha(pcm), descriptors=_sha(desc), index=_sha(idx.cpu().numpy()), y=_sha(y.cpu().numpy()))


def _record(case: str, got: dict) -> None:
    assert os.environ.get("MOVENET_HIP_LIB"), __doc__
    out = {}
    if os.path.exists(FIXTURE):
        with open(FIXTURE) as f:
            out = json.load(f)
    if out.get("recorded_from_commit") != RECORD:
        out = {"recorded_from_commit": RECORD,
               "what": "SHA-256 of the pcm and descriptor bytes (inputs) and of the index and y bytes (outputs) of "
                       "tests/test_audio_frontend_bits_gpu.py's cases, recorded on an MI355X from a library built at "
                       "that commit",
               "cases": {}}
    out["cases"][case] = got
    with open(FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


@pytest.mark.parametrize("case", list(CASES))
def test_outputs_equal_the_recording(case):
    got = run_case(case)
    if RECORD:
        _record(case, got)
        return
    with open(FIXTURE) as f:
        want = json.load(f)["cases"][case]
    print(f"{case}: " + ", ".join(f"{k} {'ok' if got[k] == want.get(k) else 'DIFFERS'}" for k in sorted(got)))
    assert (got["pcm"], got["descriptors"]) == (want["pcm"], want["descriptors"]), "the test's inputs drifted"
    assert got == want
