"""GPU: the spectral distance above the kernel -- ``WaveNet.spectral_distance`` on a tiny model (2 layers,
Q = C = K = 64, 8 mel bins, hop 16, n_fft 64 at 16 kHz; rows of 400 samples, 400 and 250 of them real), the sample
logger's two new columns, and ``python -m movenet_amd.evaluate`` end to end on two short synthetic WAVs."""
import functools
import json

import numpy as np
import pytest
import torch

import wav_material as M
from helpers import DEV, one_hot, synthetic_indices
from movenet_amd import evaluate as E
from movenet_amd import ops
from movenet_amd import synthesize as S
from movenet_amd.wavenet import SpectralDistance, WaveNet

pytestmark = pytest.mark.gpu
RECORD = {"local_channels": 8, "local_hop": 16, "mel_fft": 64, "mel_fmin": 0.0, "mel_fmax": 8000.0, "audio_rate": 16000}
T, LENGTHS = 400, [400, 250]


@functools.lru_cache(maxsize=None)
def _model():
    torch.manual_seed(11)
    m = WaveNet(2, 1, 64, 64, 64, local_channels=8, local_hop=16)
    m.local_conditioning = dict(RECORD)
    return m.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _rows():
    x = synthetic_indices(2, T, 64, 21).to(torch.int32).to(DEV)
    g = synthetic_indices(2, T, 64, 22).to(torch.int32).to(DEV)
    g[:, :_model().receptive_fields] = x[:, :_model().receptive_fields]   # a copy-synthesis keeps the prompt
    return x, g


def _mels(i):
    fbank = ops.mel_filterbank(8, 64, 16000, 0.0, 8000.0)
    return ops.logmel(i, 64, 64, 16, fbank)


def test_a_clip_is_at_distance_zero_from_itself_and_frames_follow_the_span_rule():
    m, (x, _) = _model(), _rows()
    d = m.spectral_distance(x, x, LENGTHS)
    assert isinstance(d, SpectralDistance) and d.per_frame is None
    assert d.lsd_db.dtype == torch.float64 and d.lsd_db.tolist() == [0.0, 0.0] and d.l1.tolist() == [0.0, 0.0]
    first, count = ops.distance_frame_span(LENGTHS, T, 64, 16, skip=m.receptive_fields)
    assert m.receptive_fields == 4 and (first, count) == ([3, 3], [21, 11])
    assert d.frames.dtype == torch.int32 and d.frames.tolist() == count
    assert m.spectral_distance(x, x).frames.tolist() == [21, 21]
    assert m.spectral_distance(x, x, LENGTHS, skip=0).frames.tolist() == [22, 12]
    # a prompt that reaches past the last whole window leaves nothing to compare: first = ceil(422 / 16) = 27 > F = 26
    _, g = _rows()
    none = m.spectral_distance(g, x, LENGTHS, skip=390, per_frame=True)
    assert none.frames.tolist() == [0, 0] and none.lsd_db.tolist() == [0.0, 0.0] and none.l1.tolist() == [0.0, 0.0]
    assert not none.per_frame.any()


def test_distance_is_feature_distance_of_the_two_logmels_bit_for_bit():
    m, (x, g) = _model(), _rows()
    d = m.spectral_distance(g, x, LENGTHS, per_frame=True)
    first, count = ops.distance_frame_span(LENGTHS, T, 64, 16, skip=m.receptive_fields)
    want = ops.feature_distance(_mels(g), _mels(x), first, count, per_frame=True)
    assert torch.equal(d.lsd_db, want["lsd_db"]) and torch.equal(d.l1, want["l1"])
    assert torch.equal(d.per_frame, want["per_frame"]) and torch.equal(d.frames, want["frames"])
    assert bool((d.lsd_db > 0).all()) and bool(torch.isfinite(d.lsd_db).all())
    assert not d.per_frame[:, :3].any() and not d.per_frame[1, 14:].any() and bool((d.per_frame[1, 3:14] > 0).all())
    # one-hot input goes through the model's index helper; the padding behind a row's length changes nothing
    hot = m.spectral_distance(one_hot(g.long().cpu(), 64).to(DEV), one_hot(x.long().cpu(), 64).to(DEV), LENGTHS)
    assert torch.equal(hot.lsd_db, d.lsd_db) and torch.equal(hot.l1, d.l1)
    g2 = g.clone()
    g2[1, 250:] = 0
    assert torch.equal(m.spectral_distance(g2, x, LENGTHS).lsd_db, d.lsd_db)
    # keyword arguments take the record's place
    kw = m.spectral_distance(g, x, LENGTHS, n_fft=32)
    assert kw.frames.tolist() == ops.distance_frame_span(LENGTHS, T, 32, 16, skip=4)[1]


def test_a_model_without_the_record_is_refused_and_takes_the_keywords():
    x, g = _rows()
    plain = WaveNet(2, 1, 64, 64, 64).to(DEV)
    with pytest.raises(ValueError, match="n_fft, hop, n_mels, rate"):
        plain.spectral_distance(g, x)
    got = plain.spectral_distance(g, x, LENGTHS, n_fft=64, hop=16, n_mels=8, rate=16000, f_min=0.0, f_max=8000.0)
    assert torch.equal(got.lsd_db, _model().spectral_distance(g, x, LENGTHS).lsd_db)
    with pytest.raises(ValueError, match="agree"):
        _model().spectral_distance(g[:, :300], x)
    with pytest.raises(ValueError, match="lengths"):
        _model().spectral_distance(g, x, [400])
    with pytest.raises(RuntimeError, match="no CPU path"):
        _model().spectral_distance(g.cpu(), x.cpu())


# ---- the sample logger ----------------------------------------------------------------------------------------------------

def _logged_run(tmp_path, monkeypatch, use_mel):
    from movenet_amd.callbacks import LogSamplesCallback
    from movenet_amd.config import ModelConfig, TrainingConfig
    from movenet_amd.pytorch_lightning_trainer import train_model
    seen = []
    inner = LogSamplesCallback.log_samples

    def spy(self, split, trainer, pl_module, outputs, batch, batch_idx):
        if outputs.get("generated_output", None) is not None:
            audio, *_ = batch
            n = min(int(outputs["generated_output"].shape[2]), int(audio.shape[2]))
            seen.append((pl_module.model, outputs["generated_output"][:, :, :n].argmax(1), audio[:, :, :n].argmax(1)))
        return inner(self, split, trainer, pl_module, outputs, batch, batch_idx)
    monkeypatch.setattr(LogSamplesCallback, "log_samples", spy)
    mc = ModelConfig(layer_size=2, stack_size=2, input_channels=64, residual_channels=32, skip_channels=32)
    mel = dict(use_mel=True, mel_bins=8, mel_fft=64, mel_hop=16) if use_mel else {}
    cfg = TrainingConfig(model_config=mc, batch_size=2, val_batch_size=2, n_epochs=1, n_steps_per_epoch=1, use_video=False,
                         scheduler=None, model_output_path=tmp_path, log_samples_every=1, generate_temperature=1.0,
                         score_samples=True, **mel)
    train_model("synthetic://clips=4,frames=200,seed=2", cfg)
    rows = [json.loads(line) for line in open(tmp_path / "samples" / "index.jsonl")]
    return [r for r in rows if "gen_audio" in r], seen


def test_logged_rows_carry_the_distance_of_the_clip_from_its_source(tmp_path, monkeypatch):
    rows, seen = _logged_run(tmp_path, monkeypatch, True)
    assert rows and seen
    want_db, want_l1 = [], []
    for model, gen, src in seen:
        d = model.spectral_distance(gen, src.to(gen.device))
        assert bool((d.frames > 0).all())
        want_db += d.lsd_db.tolist()
        want_l1 += d.l1.tolist()
    assert [r["mel_distance_db"] for r in rows] == want_db and [r["mel_l1"] for r in rows] == want_l1
    assert all(np.isfinite(r["mel_distance_db"]) and np.isfinite(r["mel_l1"]) and np.isfinite(r["bits_per_sample"])
               for r in rows)
    assert any(r["mel_distance_db"] > 0 for r in rows)


def test_logged_rows_without_mel_stay_as_they_were(tmp_path, monkeypatch):
    rows, _ = _logged_run(tmp_path, monkeypatch, False)
    assert rows and all("mel_distance_db" not in r and "mel_l1" not in r and "bits_per_sample" in r for r in rows)


# ---- python -m movenet_amd.evaluate ---------------------------------------------------------------------------------------

SMALL = dict(layer_size=3, stack_size=2, input_channels=64, residual_channels=16, skip_channels=8)
RECORD8 = {"local_channels": 8, "local_hop": 16, "mel_fft": 64, "mel_fmin": 0.0, "mel_fmax": 4000.0, "audio_rate": 8000}
CLIPS = (("a_8k_mono", 8000, 1500, 1), ("b_22k_stereo", 22050, 3000, 2))


def test_evaluate_end_to_end(tmp_path, capsys):
    from movenet_amd.checkpoint import load_into
    src = tmp_path / "src"
    src.mkdir()
    for seed, (name, rate, frames, channels) in enumerate(CLIPS):
        M.write_wav(str(src / f"{name}.wav"), M.quantise(M.signal("sines", rate, frames, channels, seed), 2), rate)
    torch.manual_seed(13)
    ck = WaveNet(**SMALL, local_channels=8, local_hop=16)
    torch.save({"state_dict": {f"model.{k}": v for k, v in ck.state_dict().items()},
                "local_conditioning": dict(RECORD8)}, tmp_path / "mel.ckpt")
    flags = [s for k, v in SMALL.items() for s in (f"--{k}", str(v))]
    argv = ["--checkpoint", str(tmp_path / "mel.ckpt"), "--wavs", str(src), "--device", DEV, "--batch", "2"] + flags
    assert E.main(argv + ["--synthesize", "1", "--seed", "7", "--out", str(tmp_path / "report.jsonl")]) == 0
    lines = [json.loads(ln) for ln in capsys.readouterr().out.strip().splitlines()]
    assert lines == [json.loads(ln) for ln in open(tmp_path / "report.jsonl")]
    assert len(lines) == 3 and set(lines[-1]) == {"files", "bits_per_sample", "mel_distance_db"}
    # the same calls by hand
    m = WaveNet(**SMALL).to(DEV)
    load_into(m, tmp_path / "mel.ckpt")
    m.eval()
    files = sorted(str(p) for p in src.glob("*.wav"))
    idx, lengths, feats = S.wav_batch(m, RECORD8, files, DEV)
    assert lengths == [1500, int(round(3000 * 8000 / 22050))]
    rf = m.receptive_fields
    audio = one_hot(idx.long().cpu(), 64).to(DEV)
    res = m.score(audio, lengths=lengths, local_features=feats)
    m.generate_sampling, m.generate_seed, m.generate_local_features = "model", 7, feats
    gen = m.generate(audio[:, :, :rf], n_samples=int(idx.shape[1]), temperature=1.0)
    dist = m.spectral_distance(gen, idx, lengths=lengths)
    own = m.score(gen, lengths=lengths, local_features=feats)
    for b, (rec, f) in enumerate(zip(lines[:2], files)):
        assert rec["path"] == f and rec["samples"] == lengths[b] and rec["seconds"] == lengths[b] / 8000
        assert rec["bits_per_sample"] == res.bits_per_sample[b].item() and rec["accuracy"] == res.accuracy[b].item()
        assert rec["positions"] == lengths[b] - rf
        assert rec["mel_distance_db"] == dist.lsd_db[b].item() and rec["mel_l1"] == dist.l1[b].item()
        assert rec["frames"] == dist.frames[b].item() > 0
        assert rec["generated_bits_per_sample"] == own.bits_per_sample[b].item()
        assert np.isfinite(rec["bits_per_sample"]) and rec["mel_distance_db"] > 0
    pos, frames = [r["positions"] for r in lines[:2]], [r["frames"] for r in lines[:2]]
    assert lines[2]["files"] == 2
    assert lines[2]["bits_per_sample"] == sum(r["bits_per_sample"] * p for r, p in zip(lines, pos)) / sum(pos)
    assert lines[2]["mel_distance_db"] == sum(r["mel_distance_db"] * n for r, n in zip(lines, frames)) / sum(frames)
    # without --synthesize: the same scores, no distance
    assert E.main(argv) == 0
    plain = [json.loads(ln) for ln in capsys.readouterr().out.strip().splitlines()]
    assert [r["bits_per_sample"] for r in plain] == [r["bits_per_sample"] for r in lines]
    assert all("mel_distance_db" not in r for r in plain[:2]) and plain[2]["mel_distance_db"] is None
