"""GPU: streamed synthesis -- mvn_pcm16_chunk against the sample logger's own conversion, exhaustively in
the class and on a layout with odd strides and offsets; ``WaveNet.generate_stream`` against ``generate()`` to the bit;
the generators' ``stream`` against ``advance``; and ``python -m movenet_amd.synthesize`` against ``generate()`` +
``write_wav``.  Every comparison is exact: the PCM of a class is a function of the class alone."""
import functools
import os

import numpy as np
import pytest
import torch

import wav_material as M
from helpers import DEV, one_hot, synthetic_indices
from movenet_amd import _native as N
from movenet_amd import ops
from movenet_amd import synthesize as S
from movenet_amd.callbacks import write_wav
from movenet_amd.generation import GroupedGenerator, RingGenerator, auto_plan
from movenet_amd.utils.weights import make_state_dict
from movenet_amd.wavenet import WaveNet

pytestmark = pytest.mark.gpu
SENTINEL = -32768   # never a PCM value: the conversion clips to [-32767, 32767]


def _host_pcm(waveform) -> np.ndarray:
    """The conversion of callbacks.write_wav, restated: float64, clip, x 32767, round half to even."""
    return (np.clip(np.asarray(waveform, dtype=np.float64), -1.0, 1.0) * 32767.0).round().astype("<i2")


@functools.lru_cache(maxsize=None)
def _table(Q):
    """PCM of every class 0 .. Q-1 by the host path: ops.mu_law_decode on the GPU, write_wav's conversion on the host."""
    classes = torch.arange(Q, dtype=torch.int32, device=DEV)
    return _host_pcm(ops.mu_law_decode(classes, Q).cpu().numpy())


# ---- 1. the PCM kernel ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Q", [64, 128, 256])
def test_pcm_of_every_class_is_the_wav_writers(Q, tmp_path):
    classes = torch.arange(Q, dtype=torch.int32, device=DEV)[None, :]
    got = ops.pcm16_chunk(classes, 0, Q, Q).cpu().numpy()[0]
    want = _table(Q)
    assert got.dtype == np.int16 and np.array_equal(got, want)
    assert want[0] == -32767 and want[Q - 1] == 32767 and np.all(np.diff(want.astype(np.int64)) > 0)
    # ... and it is what write_wav puts into a file
    write_wav(tmp_path / "all.wav", ops.mu_law_decode(classes[0], Q).cpu().numpy(), 8000)
    import wave
    with wave.open(str(tmp_path / "all.wav"), "rb") as w:
        stored = np.frombuffer(w.readframes(Q), dtype="<i2")
    assert np.array_equal(got, stored)
    # one column at a time, from every column offset: the value does not depend on where the class sits
    for t0 in (1, 2, 3, Q - 1):
        assert np.array_equal(ops.pcm16_chunk(classes, t0, Q - t0, Q).cpu().numpy()[0], want[t0:])


@pytest.mark.parametrize("t0,n", [(0, 1), (1, 2), (7, 16385), (20011 - 5, 5)])
@pytest.mark.parametrize("offset", [0, 1])
def test_layout_rows_heads_tails_and_nothing_else_written(t0, n, offset):
    Q, B, stride_in = 256, 3, 20011
    samples = synthetic_indices(B, stride_in, Q, 11).to(torch.int32).to(DEV)
    band = 64
    for pcm_stride in (n, n + 3):   # rows back to back, and with a gap of odd width: every other row starts odd
        buf = torch.full((2 * band + B * pcm_stride + 1,), SENTINEL, dtype=torch.int16, device=DEV)
        assert buf.data_ptr() % 4 == 0
        out = buf[band + offset:band + offset + B * pcm_stride].view(B, pcm_stride)
        ret = ops.pcm16_chunk(samples, t0, n, Q, out=out)
        assert tuple(ret.shape) == (B, n)
        want = np.full(buf.numel(), SENTINEL, dtype=np.int16)
        src = samples.cpu().numpy()
        for b in range(B):
            at = band + offset + b * pcm_stride
            want[at:at + n] = _table(Q)[src[b, t0:t0 + n]]
        got = buf.cpu().numpy()
        assert np.array_equal(got, want), (pcm_stride, np.flatnonzero(got != want)[:8])


def test_classes_out_of_range_clamp():
    for Q in (64, 256):
        bad = torch.tensor([[-1, Q, 2 ** 31 - 1, -2 ** 31, 0, Q - 1, Q + 1, -7]], dtype=torch.int32, device=DEV)
        got = ops.pcm16_chunk(bad, 0, 8, Q).cpu().numpy()[0]
        t = _table(Q)
        assert got.tolist() == [t[0], t[Q - 1], t[Q - 1], t[0], t[0], t[Q - 1], t[Q - 1], t[0]]


def test_ops_checks_its_views():
    x = torch.zeros(2, 10, dtype=torch.int32, device=DEV)
    for t0, n in ((-1, 2), (0, 11), (9, 2), (0, -1)):
        with pytest.raises(ValueError, match="columns"):
            ops.pcm16_chunk(x, t0, n, 64)
    with pytest.raises(ValueError, match="samples must be"):
        ops.pcm16_chunk(x.to(torch.int64), 0, 4, 64)
    with pytest.raises(ValueError, match="out must be"):
        ops.pcm16_chunk(x, 0, 4, 64, out=torch.zeros(2, 3, dtype=torch.int16, device=DEV))
    with pytest.raises(ValueError, match="classes"):
        ops.pcm16_chunk(x, 0, 4, 40000)
    assert tuple(ops.pcm16_chunk(x, 3, 0, 64).shape) == (2, 0)
    # a column view of a larger tensor, and a row block of it
    big = synthetic_indices(4, 50, 64, 3).to(torch.int32).to(DEV)
    got = ops.pcm16_chunk(big[1:3, 5:45], 2, 30, 64).cpu().numpy()
    assert np.array_equal(got, _table(64)[big[1:3, 7:37].cpu().numpy()])


# ---- 2. streaming equals one-shot, to the bit ---------------------------------------------------------------------------

SMALL = dict(layer_size=3, stack_size=2, input_channels=64, residual_channels=16, skip_channels=8)     # GENERIC
C2 = dict(layer_size=10, stack_size=3, input_channels=256, residual_channels=64, skip_channels=64)     # FOLD under AUTO
SHAPES = {"small": (SMALL, 3, 700), "c2": (C2, 2, 1300)}   # cfg, batch, samples beyond the receptive field
SAMPLED = dict(temperature=1.0, top_k=32, top_p=0.9)


@functools.lru_cache(maxsize=None)
def _model(shape, global_classes=0, local=False):
    cfg = SHAPES[shape][0]
    extra = dict(local_channels=8, local_hop=16) if local else {}
    torch.manual_seed(29)   # (global_embedding / local_conv keep their default initialisation, under this seed)
    m = WaveNet(**cfg, global_classes=global_classes, **extra)
    m.load_state_dict(make_state_dict(**cfg, seed=3, gain=1.5, head_gain=6.0), strict=False)
    return m.to(DEV).eval()


def _settings(m, sampled, seed, guidance=1.0):
    m.generate_sampling = "model"
    m.generate_top_k, m.generate_top_p = (SAMPLED["top_k"], SAMPLED["top_p"]) if sampled else (0, 1.0)
    m.generate_seed = seed
    m.generate_guidance = guidance
    return SAMPLED["temperature"] if sampled else 0.0


def _stream_and_one_shot(m, shape, chunk, sampled, labels=None, feats=None, guidance=1.0):
    cfg, B, extra = SHAPES[shape]
    Q, rf = cfg["input_channels"], m.receptive_fields
    n_total = rf + extra
    prompt = one_hot(synthetic_indices(B, rf, Q, 41), Q).to(DEV)
    T = _settings(m, sampled, 1234, guidance)
    if feats is not None:
        m.generate_local_features = feats
    whole = m.generate(prompt, None, labels, n_samples=n_total, temperature=T)
    want = ops.pcm16_chunk(whole.argmax(1).to(torch.int32), 0, n_total, Q).cpu().numpy()
    if feats is not None:
        m.generate_local_features = feats
    pieces = [(t0, pcm.copy()) for t0, pcm in m.generate_stream(prompt, None, labels, n_samples=n_total,
                                                                temperature=T, chunk=chunk)]
    return want, pieces, rf, n_total


def _check_pieces(want, pieces, rf, n_total, chunk):
    starts = [t0 for t0, _ in pieces]
    sizes = [p.shape[1] for _, p in pieces]
    new = n_total - rf
    assert starts == [0] + [rf + k for k in range(0, new, chunk)]
    assert sizes == [rf] + [min(chunk, new - k) for k in range(0, new, chunk)]
    assert all(p.dtype == np.int16 and p.shape[0] == want.shape[0] for _, p in pieces)
    got = np.concatenate([p for _, p in pieces], axis=1)
    assert got.shape == want.shape
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("chunk", [256, 1000])
@pytest.mark.parametrize("shape", ["small", "c2"])
def test_generate_stream_is_generate_to_the_bit(shape, chunk, sampled):
    m = _model(shape)
    cfg, B, _ = SHAPES[shape]
    with torch.cuda.device(DEV):
        plan = auto_plan(m._dims, B, False)
    assert plan == ("single", 0, N.GEN_FOLD if shape == "c2" else N.GEN_GENERIC)
    want, pieces, rf, n_total = _stream_and_one_shot(m, shape, chunk, sampled)
    _check_pieces(want, pieces, rf, n_total, chunk)
    if sampled:   # (a greedy run of these weights settles on one class: only the draws keep a clip moving)
        assert len(np.unique(want[:, rf:])) > 8
    assert m.last_generate_fallback is None


def test_guided_labelled_stream_is_generate_to_the_bit():
    m = _model("c2", global_classes=3)
    labels = torch.tensor([2, 0])
    want, pieces, rf, n_total = _stream_and_one_shot(m, "c2", 1000, True, labels=labels, guidance=1.5)
    _check_pieces(want, pieces, rf, n_total, 1000)
    plain, _, _, _ = _stream_and_one_shot(m, "c2", 1000, True, labels=labels, guidance=1.0)
    assert not np.array_equal(plain, want)     # the guidance was in force
    m.generate_guidance = 1.0


def test_stream_under_local_features_is_generate_to_the_bit():
    m = _model("small", local=True)
    cfg, B, extra = SHAPES["small"]
    n_total = m.receptive_fields + extra
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(B, 8, (n_total - 1) // 16 + 1, generator=g).to(DEV)
    want, pieces, rf, n_total = _stream_and_one_shot(m, "small", 256, True, feats=feats)
    _check_pieces(want, pieces, rf, n_total, 256)
    assert m.generate_local_features is None   # used up by the call, as generate() uses it up
    with pytest.raises(ValueError, match="local_features is required"):
        next(m.generate_stream(one_hot(synthetic_indices(B, rf, 64, 41), 64).to(DEV), n_samples=n_total))


def test_nothing_to_generate_and_argument_errors():
    m = _model("small")
    Q, rf = 64, m.receptive_fields
    _settings(m, False, 5)
    idx = synthetic_indices(2, rf + 4, Q, 9)
    x = one_hot(idx, Q).to(DEV)
    t = _table(Q)
    # n_samples <= RF: generate() returns zeros with the prompt copied in; its classes are the one chunk
    for n_samples, P in ((rf, rf + 4), (rf - 3, rf + 4), (rf + 9, rf - 1)):
        whole = m.generate(x[:, :, :P], n_samples=n_samples, temperature=0.0)
        pieces = list(m.generate_stream(x[:, :, :P], n_samples=n_samples, temperature=0.0))
        assert len(pieces) == 1 and pieces[0][0] == 0
        assert np.array_equal(pieces[0][1], t[whole.argmax(1).cpu().numpy()])
    with pytest.raises(ValueError, match="chunk"):
        next(m.generate_stream(x, n_samples=rf + 20, chunk=0))
    with pytest.raises(ValueError, match="one-hot"):
        next(m.generate_stream(0.5 * x, n_samples=rf + 20))
    # chunk > what is generated: the prompt and one short chunk
    pieces = list(m.generate_stream(x[:, :, :rf], n_samples=rf + 20, temperature=0.0, chunk=4000))
    assert [(t0, p.shape) for t0, p in pieces] == [(0, (2, rf)), (rf, (2, 20))]


# ---- 3. the generators' stream, the status word --------------------------------------------------------------------------

def _weights(cfg):
    return {k: v.to(DEV) for k, v in make_state_dict(**cfg, seed=3, gain=1.5, head_gain=6.0).items()
            if ".context_conv_" not in k}


def test_ring_stream_is_advance_and_leaves_the_status_word_zero():
    cfg, Q = C2, 256
    sd = _weights(cfg)
    kw = dict(state_dict=sd, batch=2, n_total=3072 + 601, device=DEV, variant=N.GEN_FOLD, temperature=1.0, seed=77,
              sampling="model", top_k=32, top_p=0.9)
    prompt = synthetic_indices(2, 3072, Q, 41).to(DEV)
    a = RingGenerator(**cfg, **kw)
    a.prime(prompt)
    a.advance(601)
    a.check_errors()
    b = RingGenerator(**cfg, **kw)
    b.prime(prompt)
    with pytest.raises(ValueError, match="chunk"):
        b.stream(601, chunk=0)
    pieces = [(t0, p.copy()) for t0, p in b.stream(601, chunk=250)]
    assert [(t0, p.shape[1]) for t0, p in pieces] == [(3072, 250), (3322, 250), (3572, 101)]
    assert b.t == a.t == 3672
    assert torch.equal(a.samples, b.samples)
    assert np.array_equal(np.concatenate([p for _, p in pieces], 1), _table(Q)[a.samples[:, 3072:].cpu().numpy()])
    word = b.status_word()
    assert word is not None and int(word[0].item()) == 0
    assert list(b.stream(10)) == []            # the buffer is full: nothing left to generate


def test_grouped_stream_is_grouped_advance():
    cfg, Q = C2, 256
    sd = _weights(cfg)
    kw = dict(state_dict=sd, batch=5, n_total=3072 + 300, device=DEV, group=2, variant=N.GEN_FOLD, temperature=1.0,
              seed=9, sampling="model")
    prompt = synthetic_indices(5, 3072, Q, 43).to(DEV)
    a = GroupedGenerator(**cfg, **kw)
    a.prime(prompt)
    a.advance(300)
    a.check_errors()
    b = GroupedGenerator(**cfg, **kw)
    b.prime(prompt)
    pieces = [(t0, p.copy()) for t0, p in b.stream(300, chunk=128)]
    assert [(t0, p.shape) for t0, p in pieces] == [(3072, (5, 128)), (3200, (5, 128)), (3328, (5, 44))]
    assert torch.equal(a.samples, b.samples)
    assert np.array_equal(np.concatenate([p for _, p in pieces], 1), _table(Q)[a.samples[:, 3072:].cpu().numpy()])
    assert all(int(g.status_word()[0].item()) == 0 for g in b.groups)


# ---- 4. the command line, end to end -------------------------------------------------------------------------------------

RECORD = {"local_channels": 8, "local_hop": 16, "mel_fft": 64, "mel_fmin": 0.0, "mel_fmax": 4000.0, "audio_rate": 8000}
CLIPS = (("a_8k_mono", 8000, 1500, 1), ("b_22k_stereo", 22050, 3000, 2), ("c_44k_stereo", 44100, 5001, 2),
         ("d_48k_mono", 48000, 4000, 1))


def test_cli_copy_synthesis_equals_generate_plus_write_wav(tmp_path, capsys):
    from movenet_amd.checkpoint import load_into
    src, out = tmp_path / "src", tmp_path / "out"
    src.mkdir()
    for seed, (name, rate, frames, channels) in enumerate(CLIPS):
        M.write_wav(str(src / f"{name}.wav"), M.quantise(M.signal("sines", rate, frames, channels, seed), 2), rate)
    torch.manual_seed(13)
    ck = WaveNet(**SMALL, local_channels=8, local_hop=16)      # randomly initialised
    torch.save({"state_dict": {f"model.{k}": v for k, v in ck.state_dict().items()},
                "local_conditioning": dict(RECORD)}, tmp_path / "mel.ckpt")
    flags = [s for k, v in SMALL.items() for s in (f"--{k}", str(v))]
    assert S.main(["--checkpoint", str(tmp_path / "mel.ckpt"), "--from_wavs", str(src), "--out", str(out),
                   "--chunk", "512", "--batch", "4", "--seed", "7", "--device", DEV] + flags) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 4 and all("samples=" in ln and "first_chunk_s=" in ln for ln in lines)
    # the non-streamed path: generate() + write_wav under the same settings
    m = WaveNet(**SMALL).to(DEV)
    load_into(m, tmp_path / "mel.ckpt")
    m.eval()
    files = sorted(str(p) for p in src.glob("*.wav"))
    idx, lengths, feats = S.wav_batch(m, RECORD, files, DEV)
    assert lengths == [int(round(f * 8000 / r)) for _, r, f, _ in CLIPS]
    rf = m.receptive_fields
    m.generate_sampling, m.generate_seed, m.generate_local_features = "model", 7, feats
    whole = m.generate(one_hot(idx[:, :rf].long(), 64), n_samples=int(idx.shape[1]), temperature=1.0)
    waves = ops.mu_law_decode(whole.argmax(1).to(torch.int32), 64).cpu().numpy()
    assert len(np.unique(whole.argmax(1)[:, rf:].cpu().numpy())) > 8
    for b, f in enumerate(files):
        got = out / os.path.basename(f)
        assert got.exists() and any(ln.startswith(str(got)) and f"samples={lengths[b]}\t" in ln for ln in lines)
        write_wav(tmp_path / "want" / os.path.basename(f), waves[b, :lengths[b]], 8000)
        assert got.read_bytes() == (tmp_path / "want" / os.path.basename(f)).read_bytes(), f
        assert _frames_of(got) == lengths[b]


def _frames_of(path) -> int:
    import wave
    with wave.open(str(path), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 8000)
        return w.getnframes()
