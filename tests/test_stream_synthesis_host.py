"""CPU: the host side of streamed synthesis -- the mvn_pcm16_chunk export and its refusals before any
launch, the chunk planner of ``RingGenerator.stream``, the incremental WAV writer against ``callbacks.write_wav``, and
the argument errors of ``python -m movenet_amd.synthesize``.  Nothing here needs a GPU."""
import ctypes
import wave

import numpy as np
import pytest
import torch

from movenet_amd import _native as N
from movenet_amd import synthesize as S
from movenet_amd.callbacks import write_wav
from movenet_amd.generation import plan_chunks


# ---- the C ABI ------------------------------------------------------------------------------------------------------

def test_library_exports_the_entry_point_and_the_abi_version_stays():
    lib = N.lib()
    assert hasattr(lib, "mvn_pcm16_chunk") and "mvn_pcm16_chunk" in N.SIGNATURES
    assert lib.mvn_abi_version() == 2


def test_host_refusals_return_bad_arg_with_a_text_before_any_launch():
    lib = N.lib()
    buf = (ctypes.c_uint8 * 64)()     # host memory: never dereferenced, every call below returns before a launch
    p = ctypes.addressof(buf)
    good = dict(samples=p, batch=1, sample_stride=100, t0=10, n=20, classes=256, pcm=p, pcm_stride=20)

    def call(**kw):
        a = {**good, **kw}
        return lib.mvn_pcm16_chunk(a["samples"], a["batch"], a["sample_stride"], a["t0"], a["n"], a["classes"],
                                   a["pcm"], a["pcm_stride"], None)

    for bad in (dict(samples=None), dict(pcm=None), dict(batch=0), dict(batch=-2), dict(n=-1), dict(t0=-1),
                dict(t0=81), dict(t0=2 ** 31 - 1, n=2 ** 31 - 1, pcm_stride=2 ** 31 - 1),  # t0 + n beyond int
                dict(sample_stride=29), dict(pcm_stride=19), dict(classes=1), dict(classes=0), dict(classes=-5),
                dict(classes=32769)):
        lib.mvn_abi_version()
        assert call(**bad) == N.MVN_ERR_BAD_ARG, bad
        assert "mvn_pcm16_chunk" in N.last_error() and "bad argument" in N.last_error(), bad
    with pytest.raises(ValueError, match="mvn_pcm16_chunk"):
        N.check(call(classes=1), "mvn_pcm16_chunk")
    assert call(n=0) == N.MVN_OK and call(n=0, t0=100, pcm_stride=0) == N.MVN_OK   # nothing to do: no launch
    assert call(n=0, pcm=None) == N.MVN_ERR_BAD_ARG       # ... but the arguments are still checked
    assert call(n=0, classes=1) == N.MVN_ERR_BAD_ARG
    assert call(n=0, t0=101) == N.MVN_ERR_BAD_ARG


def test_ops_refuses_a_cpu_tensor():
    from movenet_amd.ops import pcm16_chunk
    with pytest.raises(RuntimeError, match="no CPU path"):
        pcm16_chunk(torch.zeros(2, 8, dtype=torch.int32), 0, 8, 64)


# ---- the chunk planner ------------------------------------------------------------------------------------------------

def test_chunk_planner_boundaries():
    assert plan_chunks(8, 700, 256) == [(8, 256), (264, 256), (520, 188)]       # the last one short
    assert plan_chunks(3072, 8000, 4000) == [(3072, 4000), (7072, 4000)]        # chunk divides n_new
    assert plan_chunks(5, 7, 4000) == [(5, 7)]                                  # chunk > n_new
    assert plan_chunks(5, 1, 1) == [(5, 1)]
    assert plan_chunks(5, 0, 16) == [] and plan_chunks(5, -3, 16) == []         # nothing to generate
    for first, n_new, chunk in ((0, 1000, 1), (17, 1301, 1000), (1, 4001, 4000)):
        plan = plan_chunks(first, n_new, chunk)
        assert plan[0][0] == first and sum(n for _, n in plan) == n_new
        assert all(0 < n <= chunk for _, n in plan) and all(n == chunk for _, n in plan[:-1])
        assert all(a[0] + a[1] == b[0] for a, b in zip(plan, plan[1:]))         # back to back
    for bad in (0, -1, 2.5, True, None, "8"):
        with pytest.raises(ValueError, match="chunk"):
            plan_chunks(0, 10, bad)


# ---- the incremental WAV writer ---------------------------------------------------------------------------------------

def _stored(path):
    with wave.open(str(path), "rb") as w:
        return np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").copy()


@pytest.mark.parametrize("cuts", [(1, 2, 700, 701, 2500), (), (0, 0, 5), (2999,)])
def test_incremental_writer_equals_write_wav_of_the_whole_clip(tmp_path, cuts):
    rng = np.random.default_rng(3)
    wave_f = rng.uniform(-1.2, 1.2, size=3000)       # (beyond [-1, 1] on both sides: write_wav clips)
    wave_f[:4] = (0.5 / 32767.0, 1.5 / 32767.0, -0.5 / 32767.0, 1.0)   # ties and the top of the range
    write_wav(tmp_path / "whole.wav", wave_f, 22050)
    pcm = _stored(tmp_path / "whole.wav")
    assert pcm.size == 3000 and pcm.max() == 32767 and pcm.min() == -32767
    with S.IncrementalWav(tmp_path / "sub" / "pieces.wav", 22050) as w:
        for a, b in zip((0,) + cuts, cuts + (3000,)):
            assert w.write(pcm[a:b]) == b - a
        assert w.written == 3000 and not w.closed
    assert w.closed
    assert (tmp_path / "sub" / "pieces.wav").read_bytes() == (tmp_path / "whole.wav").read_bytes()
    # a limit drops what lies beyond it: the file is write_wav of the clip's head
    with S.IncrementalWav(tmp_path / "head.wav", 22050, limit=1000) as w:
        assert w.write(pcm[:900]) == 900 and not w.full
        assert w.write(pcm[900:2000]) == 100 and w.full and w.write(pcm[2000:]) == 0
    write_wav(tmp_path / "head_whole.wav", wave_f[:1000], 22050)
    assert (tmp_path / "head.wav").read_bytes() == (tmp_path / "head_whole.wav").read_bytes()
    with pytest.raises(ValueError, match="int16"):
        S.IncrementalWav(tmp_path / "bad.wav", 8000).write(np.zeros(4, np.float32))


# ---- the command line's argument errors ---------------------------------------------------------------------------------

FLAGS = dict(input_channels=64, residual_channels=16, skip_channels=8, layer_size=3, stack_size=2)


def _argv(ckpt, out, **flags):
    f = {**FLAGS, **flags}
    return ["--checkpoint", str(ckpt), "--out", str(out)] + [s for k, v in f.items() for s in (f"--{k}", str(v))]


@pytest.fixture(scope="module")
def checkpoints(tmp_path_factory):
    from movenet_amd.wavenet import WaveNet
    d = tmp_path_factory.mktemp("ckpt")
    plain = WaveNet(**FLAGS)
    torch.save({"state_dict": {f"model.{k}": v for k, v in plain.state_dict().items()}}, d / "plain.ckpt")
    mel = WaveNet(**FLAGS, local_channels=8, local_hop=16)
    torch.save({"state_dict": {f"model.{k}": v for k, v in mel.state_dict().items()},
                "local_conditioning": {"local_channels": 8, "local_hop": 16, "mel_fft": 64, "mel_fmin": 0.0,
                                       "mel_fmax": 4000.0, "audio_rate": 8000}}, d / "mel.ckpt")
    labelled = WaveNet(**FLAGS, global_classes=2)
    torch.save({"state_dict": {f"model.{k}": v for k, v in labelled.state_dict().items()},
                "global_classes": ["music", "speech"]}, d / "labelled.ckpt")
    return d


def _fails(argv, capsys, match):
    with pytest.raises(SystemExit) as e:
        S.main(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert match in err, err


def test_cli_wants_exactly_one_source(checkpoints, tmp_path, capsys):
    base = _argv(checkpoints / "plain.ckpt", tmp_path / "out")
    _fails(base, capsys, "exactly one of --from_wavs DIR and --seconds S")
    _fails(base + ["--from_wavs", str(tmp_path), "--seconds", "1"], capsys, "exactly one of --from_wavs DIR and --seconds S")
    assert not (tmp_path / "out").exists()


def test_cli_from_wavs_needs_a_mel_checkpoint_and_seconds_a_plain_one(checkpoints, tmp_path, capsys):
    _fails(_argv(checkpoints / "plain.ckpt", tmp_path / "out") + ["--from_wavs", str(tmp_path)], capsys,
           "no local_conditioning record")
    _fails(_argv(checkpoints / "mel.ckpt", tmp_path / "out") + ["--seconds", "1"], capsys, "give --from_wavs")
    _fails(_argv(checkpoints / "mel.ckpt", tmp_path / "out") + ["--from_wavs", str(tmp_path)], capsys, "no *.wav in")
    _fails(_argv(checkpoints / "labelled.ckpt", tmp_path / "out") + ["--seconds", "1"], capsys, "['music', 'speech']")
    _fails(_argv(checkpoints / "labelled.ckpt", tmp_path / "out") + ["--seconds", "1", "--label", "noise"], capsys,
           "['music', 'speech']")
    _fails(_argv(checkpoints / "plain.ckpt", tmp_path / "out") + ["--seconds", "1", "--label", "music"], capsys,
           "records no global_classes")


@pytest.mark.parametrize("flags,names", [
    (dict(residual_channels=32), "causal_conv.conv.weight: checkpoint (16, 64, 2), flags (32, 64, 2)"),
    (dict(input_channels=128), "causal_conv.conv.weight: checkpoint (16, 64, 2), flags (16, 128, 2)"),
    (dict(skip_channels=16), "--skip_channels 16"),
    (dict(layer_size=4), "missing from the checkpoint"),           # 6 layers in the file, 8 asked for
    (dict(stack_size=1), "not in a model of these flags"),         # ... and 3 asked for
])
def test_cli_checks_the_model_flags_against_the_state_dict(checkpoints, tmp_path, capsys, flags, names):
    argv = _argv(checkpoints / "plain.ckpt", tmp_path / "out", **flags) + ["--seconds", "1"]
    _fails(argv, capsys, "does not fit")
    with pytest.raises(SystemExit):
        S.main(argv)
    assert names in capsys.readouterr().err
