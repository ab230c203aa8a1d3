"""GPU: ``--mel_f0 1`` end to end on a folder of four short WAVs -- sine glides with a silent stretch in
the middle, about 0.5 s at 8 kHz: ``ops.local_features`` against its parts, two epochs of ``Trainer.fit`` with the two
F0 channels behind eight mel bins, the checkpoint's record and its readers, and ``synthesize`` with ``--pitch_shift``.
Everything compared here is compared bit for bit; there is no tolerance in this file."""
import math
import wave

import numpy as np
import pytest
import torch

import pitch_reference as PR
from helpers import DEV
from movenet_amd import checkpoint, ops
from movenet_amd import synthesize as S
from movenet_amd.wavenet import WaveNet

pytestmark = pytest.mark.gpu
RATE, Q, M, FFT, HOP = 8000, 64, 8, 64, 16
F_MIN, F_MAX = 60.0, 500.0
SHAPE = dict(layer_size=3, stack_size=1, input_channels=Q, residual_channels=64, skip_channels=64)
RECORD = {"local_channels": M, "local_hop": HOP, "mel_fft": FFT, "mel_fmin": 0.0, "mel_fmax": RATE / 2.0,
          "audio_rate": RATE}
F0 = {"f_min": F_MIN, "f_max": F_MAX, "f_ref": math.sqrt(F_MIN * F_MAX)}
CLIPS = (("a", 4000, 150.0, 250.0), ("b", 3600, 260.0, 180.0), ("c", 3800, 120.0, 200.0), ("d", 4000, 300.0, 220.0))
WIDTH = 4000


def _glide(n, f0, f1):
    """A sine gliding from f0 to f1 Hz with samples [0.4 n, 0.6 n) silent."""
    f = np.linspace(f0, f1, n)
    x = 0.5 * np.sin(2 * np.pi * np.cumsum(f) / RATE)
    x[int(0.4 * n):int(0.6 * n)] = 0.0
    return x


def _write(path, x):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(RATE)
        w.writeframes(np.round(x * 32767).astype("<i2").tobytes())


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    root = tmp_path_factory.mktemp("f0_wavs")
    tau_min, tau_max = ops.pitch_lags(RATE, F_MIN, F_MAX)
    for split in ("train", "valid"):
        (root / split / "a").mkdir(parents=True)
    for name, n, f0, f1 in CLIPS:
        x = _glide(n, f0, f1)
        # a condition on the inputs: the reference tracker finds voiced and unvoiced frames in every clip, and a gap
        # with voiced frames on both sides
        v = PR.track(x.astype(np.float32), FFT, HOP, tau_min, tau_max, 0.15)["voiced"][0]
        inside = np.nonzero(v)[0]
        assert v.sum() > 20 and (~v).sum() > 20 and (~v[inside[0]:inside[-1]]).sum() > 20, name
        for split in ("train", "valid"):
            _write(root / split / "a" / f"{name}.wav", x)
    return root


def _files(folder):
    return sorted(str(p) for p in (folder / "valid" / "a").glob("*.wav"))


@pytest.fixture(scope="module")
def indices(folder):
    idx, lengths = S.wav_indices(WaveNet(**SHAPE), RATE, _files(folder), DEV)
    assert lengths == [n for _, n, _, _ in CLIPS] and tuple(idx.shape) == (4, WIDTH)
    return idx, lengths


def _fit(folder, run_dir, **over):
    import movenet_amd.wavenet as W
    from movenet_amd.config import ModelConfig, TrainingConfig
    from movenet_amd.pytorch_lightning_trainer import Dance2Music, Trainer
    cfg = TrainingConfig(model_config=ModelConfig(**SHAPE), batch_size=4, val_batch_size=4, n_epochs=2, use_video=False,
                         optimizer="AdamW", learning_rate=1e-3, weight_decay=0.0, scheduler=None,
                         model_output_path=run_dir, loss_rule="model", clip_length="native", audio_rate=RATE,
                         use_mel=True, mel_bins=M, mel_fft=FFT, mel_hop=HOP, **over)
    m = Dance2Music(str(folder), cfg)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(W, "MAX_AUDIO_FRAMES", WIDTH)   # rows of 4000 samples (the width enters the loaders from here on)
        tr = Trainer(max_epochs=2, default_root_dir=run_dir, gradient_clip_val=0.0, limit_val_batches=1)
        tr.fit(m)
    assert len(tr.history) == 2 and all(math.isfinite(h["train_loss"]) for h in tr.history)
    assert math.isfinite(float(m.logged["val_loss"]))
    return m, run_dir / "checkpoints" / "last.ckpt"


@pytest.fixture(scope="module")
def trained(folder, tmp_path_factory):
    return _fit(folder, tmp_path_factory.mktemp("f0_run"), mel_f0=True)


@pytest.fixture(scope="module")
def trained_plain(folder, tmp_path_factory):
    return _fit(folder, tmp_path_factory.mktemp("mel_run"))


# ---- ops.local_features ---------------------------------------------------------------------------------------------------

def _logmel(idx):
    return ops.logmel(idx, Q, FFT, HOP, ops.mel_filterbank(M, FFT, RATE, 0.0, RATE / 2.0))


def _channels(period, **kw):
    return ops.pitch_features(period, float(RATE), F0["f_ref"], **kw)


def test_local_features_without_f0_is_logmel(indices):
    idx, _ = indices
    got = ops.local_features(idx, Q, RECORD)
    assert tuple(got.shape) == (4, M, WIDTH // HOP + 1) and torch.equal(got, _logmel(idx))
    assert torch.equal(ops.local_features(idx, Q, RECORD, shift=0.0, preemphasis=0.9), got)
    with pytest.raises(ValueError, match="pitch shift needs a checkpoint trained with --mel_f0 1"):
        ops.local_features(idx, Q, RECORD, shift=1.0)


def test_local_features_with_f0_is_logmel_then_the_track(indices):
    idx, lengths = indices
    rec = {**RECORD, "f0": F0}
    tau_min, tau_max = ops.pitch_lags(RATE, F_MIN, F_MAX)
    settings = dict(win=FFT, hop=HOP, tau_min=tau_min, tau_max=tau_max)
    got = ops.local_features(idx, Q, rec)
    F = WIDTH // HOP + 1
    assert tuple(got.shape) == (4, M + 2, F) and got.is_contiguous()
    assert torch.equal(got[:, :M], _logmel(idx))
    period = ops.pitch(idx, Q, **settings)["period"]
    assert torch.equal(got[:, M:], _channels(period))
    voiced = got[:, M + 1]
    assert bool(((voiced == 0) | (voiced == 1)).all()) and all(5 < int(v.sum()) < F - 5 for v in voiced)
    # pre-emphasis: the track is the one taken on the de-emphasised audio, the mel channels stay the indices'
    emph = ops.local_features(idx, Q, rec, preemphasis=0.9)
    heard = ops.pitch(ops.deemphasis_pcm16(idx, 0.9, Q).float() / 32768, **settings)["period"]
    assert torch.equal(emph[:, M:], _channels(heard)) and torch.equal(emph[:, :M], got[:, :M])
    # a shift moves channel M by exactly that many octaves and nothing else
    up = ops.local_features(idx, Q, rec, shift=1.0)
    assert torch.equal(up[:, M], got[:, M] + 1.0)
    assert torch.equal(up[:, :M], got[:, :M]) and torch.equal(up[:, M + 1], got[:, M + 1])
    each = ops.local_features(idx, Q, rec, shift=[0.0, 0.5, -0.5, 2.0])
    assert torch.equal(each[:, M], got[:, M] + torch.tensor([0.0, 0.5, -0.5, 2.0], device=DEV)[:, None])
    # lengths: a frame centred at or past its row's end is unvoiced, the frames in front keep their flag
    cut = ops.local_features(idx, Q, rec, lengths=lengths)
    ends = [-(-n // HOP) for n in lengths]
    masked = period.clone()
    for b, e in enumerate(ends):
        masked[b, e:] = 0.0
    assert torch.equal(cut[:, M:], _channels(masked)) and torch.equal(cut[:, :M], got[:, :M])


# ---- the trainer, the checkpoint and its readers ------------------------------------------------------------------------

def test_two_epochs_train_the_two_new_columns(trained, indices):
    module, path = trained
    model = module.model
    assert tuple(model.local_conv.weight.shape) == (64, M + 2, 1) and model.local_channels == M + 2
    idx, lengths = indices
    feats = ops.local_features(idx, Q, module.local_conditioning, lengths=lengths)
    assert torch.equal(feats, module.mel_features(model._one_hot_of(idx.contiguous(), torch.float32), lengths))
    for p in model.parameters():
        if p.grad is not None:
            p.grad.zero_()
    model.train()
    loss, _, _ = model(model._one_hot_of(idx.contiguous(), torch.float32), return_loss=True, local_features=feats,
                       lengths=lengths)
    loss.backward()
    grad = model.local_conv.weight.grad
    assert math.isfinite(loss.item()) and bool(torch.isfinite(grad).all())
    assert float(grad[:, M].abs().max()) > 0 and float(grad[:, M + 1].abs().max()) > 0
    ck = torch.load(path, weights_only=True)
    assert ck["local_conditioning"] == {**RECORD, "f0": F0}
    assert tuple(ck["state_dict"]["model.local_conv.weight"].shape) == (64, M + 2, 1)
    fresh = WaveNet(**SHAPE)
    checkpoint.load_into(fresh, path)
    assert fresh.local_channels == M + 2 and fresh.local_hop == HOP and fresh.local_conditioning["f0"] == F0
    want = {k[len("model."):]: v for k, v in ck["state_dict"].items()}
    got = fresh.state_dict()
    assert sorted(got) == sorted(want) and all(torch.equal(got[k], want[k]) for k in want)


def test_a_run_without_mel_f0_writes_the_record_it_wrote_before(trained_plain):
    module, path = trained_plain
    ck = torch.load(path, weights_only=True)
    assert ck["local_conditioning"] == RECORD and "f0" not in ck["local_conditioning"]
    assert tuple(ck["state_dict"]["model.local_conv.weight"].shape) == (64, M, 1)


# ---- synthesize ---------------------------------------------------------------------------------------------------------

def _one_file(folder, tmp_path):
    src = tmp_path / "src"
    src.mkdir()
    (src / "b.wav").write_bytes((folder / "valid" / "a" / "b.wav").read_bytes())
    return src


def _synth(path, src, out, *extra):
    assert S.main(["--checkpoint", str(path), "--from_wavs", str(src), "--out", str(out), "--chunk", "512", "--seed", "7",
                   "--device", DEV, *extra]) == 0
    return (out / "b.wav").read_bytes()


def test_copy_synthesis_whole_and_windowed_and_pitch_shift(trained, folder, tmp_path, capsys):
    _, path = trained
    src = _one_file(folder, tmp_path)
    whole = _synth(path, src, tmp_path / "whole", "--context", "whole")
    windowed = _synth(path, src, tmp_path / "windowed", "--context", "windowed")
    assert whole == windowed and len(whole) == 44 + 2 * 3600
    shifted = _synth(path, src, tmp_path / "shifted", "--pitch_shift", "12")
    assert len(shifted) == len(whole)
    capsys.readouterr()
    # what --pitch_shift 12 hands the model: channel M one octave up, everything else the unshifted features
    model = WaveNet(**SHAPE).to(DEV)
    checkpoint.load_into(model, path)
    rec = model.local_conditioning
    _, lengths, base = S.wav_batch(model, rec, [str(src / "b.wav")], DEV)
    _, _, up = S.wav_batch(model, rec, [str(src / "b.wav")], DEV, shift=12 / 12.0)
    _, _, zero = S.wav_batch(model, rec, [str(src / "b.wav")], DEV, shift=0 / 12.0)
    assert lengths == [3600] and tuple(base.shape) == (1, M + 2, 3600 // HOP + 1) and torch.equal(zero, base)
    assert torch.equal(up[:, M], base[:, M] + 1.0)
    assert torch.equal(up[:, :M], base[:, :M]) and torch.equal(up[:, M + 1], base[:, M + 1])


def test_pitch_shift_on_a_checkpoint_without_f0_is_refused(trained_plain, folder, tmp_path, capsys):
    _, path = trained_plain
    with pytest.raises(SystemExit) as e:
        S.main(["--checkpoint", str(path), "--from_wavs", str(_one_file(folder, tmp_path)), "--out",
                str(tmp_path / "out"), "--pitch_shift", "12", "--device", DEV])
    assert e.value.code == 2 and "--pitch_shift 12.0 needs a checkpoint trained with --mel_f0 1" in capsys.readouterr().err
    assert not (tmp_path / "out").exists()
