"""CPU: the host side of per-sequence sampling settings (mvn_seq_sampling, mvn_seq_sampling_check, the broadcast
helper of movenet_amd._native) and the sample logger's temperature sweep, with the generation stubbed."""
import ctypes as C
import json
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from movenet_amd import _native as N

Q = 64


def _rows(n, **over):
    arr = (N.SeqSampling * n)()
    for b in range(n):
        arr[b] = N.SeqSampling(1.0, 0, 1.0, b, 100 + b)
    for name, (b, v) in over.items():
        setattr(arr[b], name, v)
    return arr


def test_struct_layout():
    assert C.sizeof(N.SeqSampling) == 24
    offsets = {name: getattr(N.SeqSampling, name).offset for name, _ in N.SeqSampling._fields_}
    assert offsets == {"temperature": 0, "top_k": 4, "top_p": 8, "row": 12, "seed": 16}
    assert [name for name, _ in N.SeqSampling._fields_] == ["temperature", "top_k", "top_p", "row", "seed"]


@pytest.mark.parametrize("field,value", [("top_k", -1), ("top_p", 0.0), ("top_p", -0.1), ("top_p", 1.5),
                                         ("top_p", math.nan)])
def test_validator_refuses_bad_values_and_names_the_row(field, value):
    lib = N.lib()
    for bad_row in (0, 3):
        arr = _rows(5, **{field: (bad_row, value)})
        arr[4].top_k = Q + 5  # (a refused array is not normalised either)
        assert lib.mvn_seq_sampling_check(arr, 5, Q) == N.MVN_ERR_BAD_ARG
        text = N.last_error()
        assert f"row {bad_row}" in text and "top_k" in text and "top_p" in text, text
        assert arr[4].top_k == Q + 5
    # the first offending row is the one named
    arr = _rows(5, **{field: (1, value)})
    setattr(arr[3], field, value)
    assert lib.mvn_seq_sampling_check(arr, 5, Q) == N.MVN_ERR_BAD_ARG and "row 1" in N.last_error()


def test_validator_normalises_top_k_and_leaves_the_rest():
    lib = N.lib()
    arr = _rows(6)
    for b, k in enumerate((0, 1, Q - 1, Q, Q + 1, 2 ** 31 - 1)):
        arr[b].top_k = k
    arr[2].temperature, arr[3].temperature, arr[4].temperature = 0.0, -1.0, math.nan  # greedy rows: any value passes
    arr[5].seed, arr[5].row = 2 ** 64 - 1, 2 ** 32 - 1
    assert lib.mvn_seq_sampling_check(arr, 6, Q) == N.MVN_OK
    assert [arr[b].top_k for b in range(6)] == [0, 1, Q - 1, 0, 0, 0]
    assert arr[2].temperature == 0.0 and arr[3].temperature == -1.0 and math.isnan(arr[4].temperature)
    assert (arr[5].seed, arr[5].row) == (2 ** 64 - 1, 2 ** 32 - 1)
    assert [arr[b].top_p for b in range(6)] == [1.0] * 6 and [arr[b].row for b in range(5)] == list(range(5))
    assert lib.mvn_seq_sampling_check(arr, 0, Q) == N.MVN_OK
    assert lib.mvn_seq_sampling_check(None, 2, Q) == N.MVN_ERR_BAD_ARG
    assert lib.mvn_seq_sampling_check(arr, -1, Q) == N.MVN_ERR_BAD_ARG


def test_generate_seq_refuses_a_null_array_before_anything_else():
    rc = N.lib().mvn_generate_seq(N.make_dims(10, 3, 256, 64, 64), N.GEN_STREAM, None, None, None, 1, 10, 10, 1, 0, 5,
                                  None, None, None, 0, None, N.SAMPLE_MODEL, None)
    assert rc == N.MVN_ERR_BAD_ARG and "per_seq" in N.last_error()


def test_broadcast_helper():
    arr = N.seq_sampling_array(3, Q, 0.5, 8, 0.9, 7)
    assert [(e.temperature, e.top_k, round(e.top_p, 6), e.seed, e.row) for e in arr] == [
        (0.5, 8, 0.9, 7, b) for b in range(3)]
    arr = N.seq_sampling_array(3, Q, [0.0, 0.5, 1.0], torch.tensor([0, 8, Q]), np.array([1.0, 0.5, 0.25]),
                               (1, 2 ** 64 - 1, -1), rows=[5, 0, 2 ** 32 - 1])
    assert [e.temperature for e in arr] == [0.0, 0.5, 1.0]
    assert [e.top_k for e in arr] == [0, 8, 0]                  # (Q: every class kept, normalised to off)
    assert [e.top_p for e in arr] == [1.0, 0.5, 0.25]
    assert [e.seed for e in arr] == [1, 2 ** 64 - 1, 2 ** 64 - 1]  # (keys are taken modulo 2^64, like the scalar seed)
    assert [e.row for e in arr] == [5, 0, 2 ** 32 - 1]
    assert N.any_per_sequence(1.0, 0, 1.0, [1, 2]) and N.any_per_sequence(torch.tensor([1.0]))
    assert not N.any_per_sequence(1.0, 0, 1.0, 5, None, torch.tensor(1.0), np.float32(2.0))


@pytest.mark.parametrize("kw,match", [
    (dict(temperature=[1.0, 0.5]), "temperature has 2 entries for a batch of 3"),
    (dict(top_k=[1, 2, 3, 4]), "top_k has 4 entries"),
    (dict(top_p=torch.ones(2)), "top_p has 2 entries"),
    (dict(seed=[1]), "seed has 1 entries"),
    (dict(rows=[0, 1]), "rows has 2 entries"),
    (dict(temperature=torch.ones(3, 1)), "temperature must be a scalar or a 1-D sequence"),
    (dict(top_k=[0, -1, 0]), "row 1"),
    (dict(top_p=[1.0, 1.0, math.nan]), "row 2"),
    (dict(top_p=0.0), "row 0"),
    (dict(top_k=[0, 1.5, 0]), "top_k of row 1"),
    (dict(top_k=[0, True, 0]), "top_k of row 1"),
    (dict(temperature=[1.0, "hot", 1.0]), "temperature of row 1"),
    (dict(rows=[0, -1, 2]), "row 1"),
    (dict(rows=[0, 1, 2 ** 32]), "row 2"),
])
def test_broadcast_helper_refusals(kw, match):
    args = dict(temperature=1.0, top_k=0, top_p=1.0, seed=0)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        N.seq_sampling_array(3, Q, **args)


# ---- the sample logger ------------------------------------------------------------------------------------------
def _log(tmp_path, monkeypatch, sweep, n_gen):
    """One log_samples call on 2 clips of 5 samples; the "generated" waveform of row r is the constant r / 10."""
    from movenet_amd import callbacks as CB
    monkeypatch.setattr(CB.LogSamplesCallback, "_decode",
                        staticmethod(lambda t, classes: t.to(torch.float64).numpy()))  # (B, S) passed straight through
    cb = CB.LogSamplesCallback(log_every_n_epochs=1, out_dir=str(tmp_path), **({} if sweep is None else
                                                                              {"temperature_sweep": sweep}))
    trainer = SimpleNamespace(current_epoch=3, rank=0, root=None)
    module = SimpleNamespace(config=SimpleNamespace(model_config=SimpleNamespace(input_channels=Q)))
    outputs = {"output": torch.zeros(2, 5),
               "generated_output": None if n_gen is None else
               (torch.arange(n_gen, dtype=torch.float32) / 10)[:, None].repeat(1, 5)}
    batch = (torch.zeros(2, 5), None, None, ["a.mp4", "b.mp4"], None)
    cb.log_samples("validation", trainer, module, outputs, batch, 7)
    rows = [json.loads(line) for line in open(tmp_path / "index.jsonl")]
    files = sorted(p.name for p in (tmp_path / "validation").iterdir())
    return rows, files


def _pcm(path):
    import wave
    with wave.open(str(path), "rb") as w:
        return np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")


def test_logger_without_a_sweep_writes_what_it_always_wrote(tmp_path, monkeypatch):
    for sub, sweep in (("default", None), ("empty", [])):
        rows, files = _log(tmp_path / sub, monkeypatch, sweep, 2)
        stems = [f"epoch=3-batch=7-clip={i}" for i in range(2)]
        assert files == sorted(f"{s}-{kind}.wav" for s in stems for kind in ("origin", "pred", "gen"))
        assert rows == [{"split": "validation", "epoch": 3, "batch_idx": 7, "fp": fp,
                         "origin_audio": f"validation/{s}-origin.wav", "pred_audio": f"validation/{s}-pred.wav",
                         "gen_audio": f"validation/{s}-gen.wav"} for s, fp in zip(stems, ["a.mp4", "b.mp4"])]
    rows, files = _log(tmp_path / "nogen", monkeypatch, None, None)
    assert all("gen_audio" not in r and "temperature" not in r for r in rows) and len(files) == 4


def test_logger_with_a_sweep_writes_one_file_and_row_per_clip_and_temperature(tmp_path, monkeypatch):
    sweep = [0.0, 0.5, 1.25]
    rows, files = _log(tmp_path, monkeypatch, sweep, 6)
    stems = [f"epoch=3-batch=7-clip={i}" for i in range(2)]
    names = ["T0", "T0.5", "T1.25"]
    assert files == sorted([f"{s}-{kind}.wav" for s in stems for kind in ("origin", "pred")] +
                           [f"{s}-gen-{t}.wav" for s in stems for t in names])
    assert rows == [{"split": "validation", "epoch": 3, "batch_idx": 7, "fp": fp,
                     "origin_audio": f"validation/{s}-origin.wav", "pred_audio": f"validation/{s}-pred.wav",
                     "gen_audio": f"validation/{s}-gen-{name}.wav", "temperature": t}
                    for s, fp in zip(stems, ["a.mp4", "b.mp4"]) for name, t in zip(names, sweep)]
    # clip-major: row 3 i + j of the generated batch is clip i at sweep[j]
    for i, s in enumerate(stems):
        for j, name in enumerate(names):
            want = round((3 * i + j) / 10 * 32767.0)
            assert (_pcm(tmp_path / "validation" / f"{s}-gen-{name}.wav") == want).all()
    # a generated batch that is not clips x temperatures is refused
    with pytest.raises(ValueError, match="2 clips x 3 temperatures"):
        _log(tmp_path / "bad", monkeypatch, sweep, 4)
    # no generation this epoch: the sweep writes nothing of its own
    rows, files = _log(tmp_path / "nogen", monkeypatch, sweep, None)
    assert all("temperature" not in r and "gen_audio" not in r for r in rows) and len(files) == 4


def test_sweep_flag_and_config_field():
    from movenet_amd.config import TrainingConfig, arg_parser, config_from_args
    args = arg_parser().parse_args(["--dataset", "x"])
    assert args.generate_temperature_sweep == [] and config_from_args(args).generate_temperature_sweep == []
    args = arg_parser().parse_args(["--dataset", "x", "--generate_temperature_sweep", "0,0.5,1.25"])
    cfg = config_from_args(args)
    assert cfg.generate_temperature_sweep == [0.0, 0.5, 1.25]
    assert TrainingConfig.from_json(cfg.to_json()).generate_temperature_sweep == [0.0, 0.5, 1.25]
