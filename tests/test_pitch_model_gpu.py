"""GPU: the pitch distance above the kernels -- ``WaveNet.pitch_distance`` on the tiny mel model of the
local-conditioning tests (2 layers, Q = C = K = 64, 8 mel bins, hop 16, n_fft 64 at 16 kHz: lags 32 .. 267, frames of
64 + 267 samples), ``evaluate --pitch 1`` end to end on two short WAVs, and the sample logger's ``--score_pitch``."""
import functools
import json
import math

import numpy as np
import pytest
import torch

import wav_material as M
from helpers import DEV
from movenet_amd import evaluate as E
from movenet_amd import ops
from movenet_amd.types import PitchDistance
from movenet_amd.wavenet import WaveNet

pytestmark = pytest.mark.gpu
RECORD = {"local_channels": 8, "local_hop": 16, "mel_fft": 64, "mel_fmin": 0.0, "mel_fmax": 8000.0, "audio_rate": 16000}
T, P_SRC = 2000, 60.0
P_GEN = P_SRC / 2.0 ** (1.0 / 12.0)  # one semitone sharp
PITCH_KEYS = {"f0_rmse_cents", "voiced_frames", "vuv_error_rate", "gross_pitch_error_rate"}


@functools.lru_cache(maxsize=None)
def _model():
    torch.manual_seed(11)
    m = WaveNet(2, 1, 64, 64, 64, local_channels=8, local_hop=16)
    m.local_conditioning = dict(RECORD)
    return m.to(DEV).eval()


def _tone(period, rows=2):
    t = torch.arange(T, dtype=torch.float64)
    wave = torch.stack([0.8 * torch.sin(2 * math.pi * t / period + 0.3 * r) for r in range(rows)])
    return ops.mu_law_encode(wave.float().to(DEV), 64)


def test_a_tone_is_at_distance_zero_from_itself():
    m, x = _model(), _tone(P_SRC)
    d = m.pitch_distance(x, x)
    assert isinstance(d, PitchDistance)
    assert d.f0_rmse_cents.dtype == torch.float64 and d.f0_rmse_cents.tolist() == [0.0, 0.0]
    assert d.vuv_errors.tolist() == [0, 0] and d.gross_errors.tolist() == [0, 0]
    first, count = ops.distance_frame_span(None, T, 64 + 267, 16, skip=m.receptive_fields, batch=2)
    assert d.frames.tolist() == count and min(count) > 50
    assert bool((d.voiced_frames == d.frames).all())  # every frame inside the clip holds the tone
    # lengths cut the span as they cut spectral_distance's
    short = m.pitch_distance(x, x, [T, 1000])
    assert short.frames.tolist() == ops.distance_frame_span([T, 1000], T, 331, 16, skip=m.receptive_fields)[1]


def test_a_semitone_is_a_hundred_cents_within_the_trackers_resolution():
    """Each track lies within 1.5 samples of its tone's period (the integer minimum within 1, the refinement within
    1/2 of that), so every frame's error lies in 1200 log2((60 -+ 1.5) / (56.63 +- 1.5)) = [10.9, 189.2] cents, and
    their root mean square with it; no frame is a gross error at 20 % ((56.63 -+ 1.5) / (60 +- 1.5) - 1 >= -0.104)."""
    m = _model()
    d = m.pitch_distance(_tone(P_GEN), _tone(P_SRC))
    lo = 1200 * math.log2((P_SRC - 1.5) / (P_GEN + 1.5))
    hi = 1200 * math.log2((P_SRC + 1.5) / (P_GEN - 1.5))
    print("semitone:", d.f0_rmse_cents.tolist(), "bounds", lo, hi)
    assert bool((d.voiced_frames == d.frames).all()) and d.vuv_errors.tolist() == [0, 0]
    assert all(lo <= v <= hi for v in d.f0_rmse_cents.tolist())
    assert d.gross_errors.tolist() == [0, 0]
    # an octave apart is a gross error in every frame
    octave = m.pitch_distance(_tone(2 * P_SRC), _tone(P_SRC))
    assert octave.gross_errors.tolist() == octave.voiced_frames.tolist() and min(octave.voiced_frames.tolist()) > 50


def test_under_preemphasis_both_sides_are_tracked_on_the_deemphasised_audio():
    x, g = _tone(P_SRC), _tone(P_GEN)
    torch.manual_seed(11)
    m = WaveNet(2, 1, 64, 64, 64, local_channels=8, local_hop=16).to(DEV).eval()
    m.local_conditioning = dict(RECORD)
    m.preemphasis = 0.97
    d = m.pitch_distance(g, x, [T, 1500])
    kw = dict(win=64, hop=16, tau_min=32, tau_max=267, threshold=0.15)
    tracks = [ops.pitch(ops.deemphasis_pcm16(i, m.preemphasis, 64).float() / 32768, **kw)["period"] for i in (g, x)]
    first, count = ops.distance_frame_span([T, 1500], T, 331, 16, skip=m.receptive_fields)
    want = ops.pitch_distance(tracks[0], tracks[1], first, count)
    assert torch.equal(d.f0_rmse_cents, want["f0_rmse_cents"]) and torch.equal(d.voiced_frames, want["voiced_frames"])
    assert torch.equal(d.vuv_errors, want["vuv_errors"]) and torch.equal(d.frames, want["frames"])
    # ... which is not the track of the class indices themselves
    plain = ops.pitch(g, 64, **kw)["period"]
    assert not torch.equal(plain, tracks[0])
    # keywords take the record's place, and a model without the record needs them
    bare = WaveNet(2, 1, 64, 64, 64).to(DEV)
    with pytest.raises(ValueError, match="win, hop and rate"):
        bare.pitch_distance(g, x)
    got = bare.pitch_distance(g, x, [T, 1500], win=64, hop=16, rate=16000)
    assert torch.equal(got.frames, d.frames)
    assert torch.equal(got.f0_rmse_cents, _model().pitch_distance(g, x, [T, 1500]).f0_rmse_cents)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _model().pitch_distance(g.cpu(), x.cpu())


# ---- python -m movenet_amd.evaluate ---------------------------------------------------------------------------------------

SMALL = dict(layer_size=3, stack_size=2, input_channels=64, residual_channels=16, skip_channels=8)
RECORD8 = {"local_channels": 8, "local_hop": 16, "mel_fft": 64, "mel_fmin": 0.0, "mel_fmax": 4000.0, "audio_rate": 8000}
CLIPS = (("a_8k_mono", 8000, 1500, 1), ("b_22k_stereo", 22050, 3000, 2))


def test_evaluate_writes_the_pitch_figures_and_leaves_the_other_lines_as_they_were(tmp_path, capsys):
    from movenet_amd import synthesize as S
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
    argv = ["--checkpoint", str(tmp_path / "mel.ckpt"), "--wavs", str(src), "--device", DEV, "--batch", "2",
            "--synthesize", "1", "--seed", "7"] + flags
    assert E.main(argv) == 0
    before = capsys.readouterr().out.strip().splitlines()
    assert E.main(argv + ["--pitch", "1", "--pitch_fmin", "80", "--pitch_fmax", "400"]) == 0
    after = capsys.readouterr().out.strip().splitlines()
    assert len(before) == len(after) == 3
    lines = [json.loads(ln) for ln in after]
    for old, new in zip(before, lines):  # without the flag: the bytes of the lines with the new keys taken out
        assert PITCH_KEYS.isdisjoint(json.loads(old))
        assert old == json.dumps({k: v for k, v in new.items() if k not in PITCH_KEYS})
    assert all(PITCH_KEYS <= set(r) for r in lines[:2])
    assert {"f0_rmse_cents", "vuv_error_rate", "gross_pitch_error_rate"} <= set(lines[2]) and "voiced_frames" not in lines[2]
    # the same calls by hand
    m = WaveNet(**SMALL).to(DEV)
    load_into(m, tmp_path / "mel.ckpt")
    m.eval()
    files = sorted(str(p) for p in src.glob("*.wav"))
    idx, lengths, feats = S.wav_batch(m, RECORD8, files, DEV)
    rf = m.receptive_fields
    audio = m._one_hot_of(idx.contiguous(), torch.float32)
    m.generate_sampling, m.generate_seed, m.generate_local_features = "model", 7, feats
    gen = m.generate(audio[:, :, :rf], n_samples=int(idx.shape[1]), temperature=1.0)
    d = m.pitch_distance(gen, idx, lengths=lengths, f_min=80.0, f_max=400.0)
    assert bool((d.frames > 0).all())
    both, vuv, gross, frames = (t.tolist() for t in (d.voiced_frames, d.vuv_errors, d.gross_errors, d.frames))
    for b, rec in enumerate(lines[:2]):
        assert rec["voiced_frames"] == both[b] and rec["vuv_error_rate"] == vuv[b] / frames[b]
        assert rec["f0_rmse_cents"] == (d.f0_rmse_cents[b].item() if both[b] else None)
        assert rec["gross_pitch_error_rate"] == (gross[b] / both[b] if both[b] else None)
    assert lines[2]["vuv_error_rate"] == sum(vuv) / sum(frames)
    assert lines[2]["gross_pitch_error_rate"] == (sum(gross) / sum(both) if sum(both) else None)
    square = sum((r["f0_rmse_cents"] or 0.0) ** 2 * r["voiced_frames"] for r in lines[:2])
    assert lines[2]["f0_rmse_cents"] == ((square / sum(both)) ** 0.5 if sum(both) else None)


# ---- the sample logger ----------------------------------------------------------------------------------------------------

def _logged_run(out, monkeypatch, score_pitch):
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
    # at 16 kHz the lags of 60 .. 500 Hz are 32 .. 267: 17 frames of 64 + 267 samples lie inside a clip of 600
    cfg = TrainingConfig(model_config=mc, batch_size=2, val_batch_size=2, n_epochs=1, n_steps_per_epoch=1, use_video=False,
                         scheduler=None, model_output_path=out, log_samples_every=1, generate_temperature=0.0,
                         score_samples=True, score_pitch=score_pitch, use_mel=True, mel_bins=8, mel_fft=64, mel_hop=16)
    torch.manual_seed(5)
    train_model("synthetic://clips=4,frames=600,seed=2", cfg)
    rows = [json.loads(line) for line in open(out / "samples" / "index.jsonl")]
    return [r for r in rows if "gen_audio" in r], seen


def test_logged_rows_gain_the_pitch_figures_only_with_score_pitch(tmp_path, monkeypatch):
    keys = ("f0_rmse_cents", "vuv_error_rate", "gross_pitch_error_rate")
    (tmp_path / "on").mkdir()
    (tmp_path / "off").mkdir()
    rows, seen = _logged_run(tmp_path / "on", monkeypatch, True)
    monkeypatch.undo()
    plain, _ = _logged_run(tmp_path / "off", monkeypatch, False)
    assert rows and seen and len(plain) == len(rows)
    assert all(set(keys) <= set(r) for r in rows) and all(set(keys).isdisjoint(r) for r in plain)
    assert [{k: v for k, v in r.items() if k not in keys} for r in rows] == plain  # every other field as it was
    want = {k: [] for k in keys}
    for model, gen, src in seen:
        d = model.pitch_distance(gen, src.to(gen.device))
        assert bool((d.frames > 0).all())
        for b in range(int(gen.shape[0])):
            both, f = d.voiced_frames[b].item(), d.frames[b].item()
            want["f0_rmse_cents"].append(d.f0_rmse_cents[b].item() if both else None)
            want["vuv_error_rate"].append(d.vuv_errors[b].item() / f)
            want["gross_pitch_error_rate"].append(d.gross_errors[b].item() / both if both else None)
    for k in keys:
        assert [r[k] for r in rows] == want[k], k
