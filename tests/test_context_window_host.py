"""CPU: the windowed generator context as far as it needs no GPU -- the three exports are bound from the
header, every refusal of mvn_generate_windowed comes back with its code and text on dummy pointers (nothing is
launched: each call carries at least one refusal), ``synthesize --context auto`` and the ValueErrors of
``generate_stream(context=...)``."""
import ctypes

import pytest
import torch

from movenet_amd import _native as N
from movenet_amd import synthesize as S
from movenet_amd.wavenet import WaveNet

D2 = dict(layer_size=10, stack_size=3, input_channels=256, residual_channels=64, skip_channels=64)
PTR = 0x10000  # a pointer that is never followed: every call below is refused before a launch


def test_the_three_exports_are_bound_from_the_header():
    lib = N.lib()
    for name, n_args in (("mvn_generate_windowed", 25), ("mvn_project_features", 12), ("mvn_context_window", 12)):
        assert name in N.SIGNATURES, name
        res, args = N.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == n_args
        assert getattr(lib, name).argtypes == args
    # the DEVICE array of per-sequence settings is an address, not a host struct
    names = ["dims", "variant", "packed", "state", "samples", "batch", "sample_stride", "n_total", "n_given", "t_begin",
             "t_end", "temperature", "seed", "top_k", "top_p", "per_seq", "guidance", "logits_out", "choices_out",
             "logits_t0", "context_win", "ctx_t0", "ctx_len", "sampling", "stream"]
    args = N.SIGNATURES["mvn_generate_windowed"][1]
    assert args[names.index("per_seq")] is ctypes.c_void_p
    assert args[names.index("seed")] is ctypes.c_uint64 and args[names.index("top_p")] is ctypes.c_float
    assert lib.mvn_abi_version() == N.ABI_VERSION == 2


def _windowed(variant=N.GEN_GENERIC, packed=PTR, state=PTR, samples=PTR, batch=2, stride=100, n_total=100, n_given=10,
              t=(10, 20), temperature=0.0, seed=0, top_k=0, top_p=1.0, per_seq=None, guidance=None, logits_t0=0,
              win=PTR, ctx_t0=10, ctx_len=10, sampling=N.SAMPLE_MODEL, dims=None):
    dims = N.make_dims(**D2) if dims is None else dims
    rc = N.lib().mvn_generate_windowed(dims, variant, packed, state, samples, batch, stride, n_total, n_given, t[0], t[1],
                                       temperature, seed, top_k, top_p, per_seq, guidance, None, None, logits_t0, win,
                                       ctx_t0, ctx_len, sampling, None)
    return rc, N.last_error()


@pytest.mark.parametrize("kw", [
    dict(win=None),
    dict(ctx_len=0),
    dict(ctx_len=-3),
    dict(ctx_t0=-1, ctx_len=40),
    dict(ctx_t0=11, ctx_len=9),    # one column short in front: [11, 20) against the launch's [10, 20)
    dict(ctx_t0=10, ctx_len=9),    # one column short behind: [10, 19)
    dict(ctx_t0=11, ctx_len=20),   # long enough, but it starts late
    dict(ctx_t0=0, ctx_len=19),
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_a_window_that_does_not_hold_the_launchs_columns_is_refused_first(kw):
    # (every later refusal is planted too: the window's comes first)
    rc, text = _windowed(packed=None, sampling=7, top_k=-1, variant=N.GEN_AUTO, **kw)
    assert rc == N.MVN_ERR_BAD_ARG
    assert text.startswith("mvn_generate_windowed: bad argument") and "columns [10, 20)" in text
    if kw.get("win", PTR) is None:
        assert "is NULL" in text
    else:
        t0, n = kw.get("ctx_t0", 10), kw.get("ctx_len", 10)
        assert f"holds columns [{t0}, {t0 + n})" in text


def test_a_window_that_just_holds_them_passes_on_to_the_next_refusal():
    for t0, n in ((10, 10), (0, 20), (9, 12), (10, 2 ** 31 - 1)):   # (the last: ctx_t0 + ctx_len beyond an int)
        rc, text = _windowed(ctx_t0=t0, ctx_len=n, sampling=7)
        assert rc == N.MVN_ERR_BAD_ARG and "sampling 7" in text, (t0, n, text)
    # an empty launch lies inside any window
    rc, text = _windowed(t=(10, 10), ctx_t0=50, ctx_len=1, sampling=7)
    assert rc == N.MVN_ERR_BAD_ARG and "sampling 7" in text


def test_the_refusals_of_the_three_calls_it_stands_for_in_their_order():
    # scalar path (per_seq NULL): mvn_generate_trunc's
    rc, text = _windowed(variant=N.GEN_AUTO, sampling=7, top_k=-1, packed=None)
    assert rc == N.MVN_ERR_BAD_ARG and "resolve the variant" in text
    rc, text = _windowed(sampling=7, top_k=-1, packed=None)
    assert rc == N.MVN_ERR_BAD_ARG and "sampling 7" in text
    rc, text = _windowed(top_k=-1, packed=None)
    assert rc == N.MVN_ERR_BAD_ARG and "top_k -1" in text
    rc, text = _windowed(top_p=float("nan"), packed=None)
    assert rc == N.MVN_ERR_BAD_ARG and "top_p" in text
    rc, text = _windowed(variant=N.GEN_PIPE_F16, packed=None)     # config 2's dims have no PIPE_F16
    assert rc == N.MVN_ERR_UNSUPPORTED
    rc, text = _windowed(dims=N.make_dims(0, 3, 256, 64, 64), packed=None)
    assert rc == N.MVN_ERR_BAD_DIMS
    for kw in (dict(packed=None), dict(state=None), dict(samples=None), dict(batch=-1), dict(stride=99),
               dict(n_given=0), dict(n_given=101), dict(logits_t0=101), dict(logits_t0=-1)):
        rc, text = _windowed(**kw)
        assert rc == N.MVN_ERR_BAD_ARG and text.startswith("mvn_generate: bad argument"), (kw, text)
    rc, text = _windowed(t=(20, 10), ctx_t0=0, ctx_len=100)        # (t_end < t_begin: an empty launch to the window check)
    assert rc == N.MVN_ERR_BAD_ARG and "t [20,10)" in text
    rc, text = _windowed(t=(95, 101), ctx_t0=90, ctx_len=20)       # inside the window, beyond n_total
    assert rc == N.MVN_ERR_BAD_ARG and "t [95,101)" in text
    # per_seq given: the scalars are not read (a bad top_k passes), the driver's checks follow
    rc, text = _windowed(per_seq=PTR, top_k=-1, packed=None)
    assert rc == N.MVN_ERR_BAD_ARG and text.startswith("mvn_generate: bad argument")
    # guidance given: mvn_generate_guided's, before the driver's
    rc, text = _windowed(guidance=PTR, per_seq=None, sampling=7)
    assert rc == N.MVN_ERR_BAD_ARG and "mvn_generate_guided" in text and "per_seq is NULL" in text
    rc, text = _windowed(guidance=PTR, per_seq=PTR, batch=0, sampling=7)
    assert rc == N.MVN_ERR_BAD_ARG and "pairs 0" in text
    rc, text = _windowed(guidance=PTR, per_seq=PTR, variant=N.GEN_AUTO, sampling=7)
    assert rc == N.MVN_ERR_BAD_ARG and "resolve the variant" in text
    limit = N.lib().mvn_gen_guided_max_pairs(N.make_dims(**D2), N.GEN_FOLD)
    rc, text = _windowed(guidance=PTR, per_seq=PTR, variant=N.GEN_FOLD, batch=limit + 1, sampling=7)
    assert rc == N.MVN_ERR_UNSUPPORTED and f"at most {limit} pairs" in text
    rc, text = _windowed(guidance=PTR, per_seq=PTR, variant=N.GEN_STREAM, sampling=7)   # no guided form
    assert rc == N.MVN_ERR_UNSUPPORTED
    rc, text = _windowed(guidance=PTR, per_seq=PTR, variant=N.GEN_FOLD, batch=2, sampling=7)
    assert rc == N.MVN_ERR_BAD_ARG and "sampling 7" in text
    with pytest.raises(ValueError, match="columns"):
        N.check(_windowed(win=None)[0], "mvn_generate_windowed")


def test_context_window_and_project_features_refuse_before_any_launch():
    lib = N.lib()

    def window(proj=PTR, proj_ld=10, proj_rows=2, frames=10, glob=PTR, rows=2, C=16, hop=7, t0=0, n=8, win=PTR):
        return lib.mvn_context_window(proj, proj_ld, proj_rows, frames, glob, rows, C, hop, t0, n, win, None), N.last_error()

    for kw, word in ((dict(win=None), "win is NULL"), (dict(proj=None, glob=None), "both NULL"), (dict(rows=-1), "below 1"),
                     (dict(C=0), "below 1"), (dict(n=0), "below 1"), (dict(t0=-1), "negative"), (dict(rows=65536), "65535"),
                     (dict(C=65536), "65535"), (dict(t0=2 ** 30, n=1, frames=2 ** 30), "2^30"),
                     (dict(proj_rows=0), "below 1"), (dict(frames=0), "below 1"), (dict(hop=0), "below 1"),
                     (dict(proj_ld=9), "proj_ld"), (dict(hop=2 ** 24 + 1, frames=10), "2^24"),
                     (dict(frames=2 ** 30 + 1, proj_ld=2 ** 30 + 1), "2^30")):
        rc, text = window(**kw)
        assert rc == N.MVN_ERR_BAD_ARG and text.startswith("mvn_context_window") and word in text, (kw, text)
    # frames: 10 at hop 7 reach column 69 (j = 9); column 70 needs an eleventh
    rc, text = window(t0=62, n=9)
    assert rc == N.MVN_ERR_BAD_ARG and "too few frames for columns [62, 71)" in text
    assert window(rows=0)[0] == N.MVN_OK                     # nothing to do, nothing launched
    assert window(rows=0, proj=None)[0] == N.MVN_OK          # (a label alone: no frame arithmetic is checked)

    def project(mel=PTR, mel_ld=10, w=PTR, bias=PTR, batch=2, M=5, F=10, C=16, taps=3, proj=PTR, proj_ld=10):
        return lib.mvn_project_features(mel, mel_ld, w, bias, batch, M, F, C, taps, proj, proj_ld, None), N.last_error()

    for kw, word in ((dict(mel=None), "null pointer"), (dict(w=None), "null pointer"), (dict(bias=None), "null pointer"),
                     (dict(proj=None), "null pointer"), (dict(taps=2), "taps"), (dict(taps=0), "taps"),
                     (dict(taps=35), "taps"), (dict(batch=-1), "below 1"), (dict(M=0), "below 1"), (dict(F=0), "below 1"),
                     (dict(C=0), "below 1"), (dict(batch=65536), "65535"), (dict(F=2 ** 30 + 1, mel_ld=2 ** 30 + 1,
                                                                                 proj_ld=2 ** 30 + 1), "2^30"),
                     (dict(mel_ld=9), "row stride"), (dict(proj_ld=9), "row stride")):
        rc, text = project(**kw)
        assert rc == N.MVN_ERR_BAD_ARG and text.startswith("mvn_project_features") and word in text, (kw, text)
    assert project(batch=0)[0] == N.MVN_OK


def test_synthesize_context_auto_takes_windowed_above_one_gibibyte():
    # config 2, 16 sequences: 2 x 16 x 64 x 4 = 8 KiB per column, so 2^17 columns are exactly 1 GiB
    assert S.whole_context_bytes(16, 64, 1) == 8192
    assert S.whole_context_bytes(16, 64, 1 << 17) == 1 << 30 == S.WHOLE_CONTEXT_LIMIT
    assert S.context_mode("auto", True, 16, 64, 1 << 17) == "whole"            # exactly 1 GiB: not above it
    assert S.context_mode("auto", True, 16, 64, (1 << 17) + 1) == "windowed"
    assert S.context_mode("auto", True, 16, 64, 9_600_000) == "windowed"       # the ten-minute file
    assert S.context_mode("auto", True, 1, 64, 57_600_000) == "windowed"       # one hour from a label
    assert S.context_mode("auto", True, 16, 64, 16000) == "whole"
    assert S.context_mode("auto", True, 32, 64, 1 << 16) == "whole"            # (guided: twice the rows)
    assert S.context_mode("auto", True, 32, 64, (1 << 16) + 1) == "windowed"
    assert S.context_mode("auto", False, 16, 64, 10 ** 9) == "whole"           # unconditioned: no context is built
    for flag in ("whole", "windowed"):
        assert S.context_mode(flag, True, 16, 64, 10 ** 9) == flag
        assert S.context_mode(flag, True, 1, 64, 10) == flag
    args = S.build_parser().parse_args(["--checkpoint", "x", "--out", "y"])
    assert args.context == "auto"
    assert S.build_parser().parse_args(["--checkpoint", "x", "--out", "y", "--context", "windowed"]).context == "windowed"
    with pytest.raises(SystemExit):
        S.build_parser().parse_args(["--checkpoint", "x", "--out", "y", "--context", "sliding"])


def test_generate_stream_refuses_windowed_with_video_and_unknown_modes():
    m = WaveNet(layer_size=2, stack_size=2, input_channels=64, residual_channels=16, skip_channels=16)
    audio = torch.zeros(1, 64, 8)
    audio[:, 0] = 1.0
    with pytest.raises(ValueError, match="windowed.*video"):
        next(m.generate_stream(audio, video=torch.zeros(1, 1, 64, 64, 1), n_samples=20, context="windowed"))
    with pytest.raises(ValueError, match="'whole' or 'windowed'"):
        next(m.generate_stream(audio, n_samples=20, context="sliding"))
    with pytest.raises(ValueError, match="chunk"):   # (the chunk's check still comes first)
        next(m.generate_stream(audio, n_samples=20, chunk=0, context="sliding"))
