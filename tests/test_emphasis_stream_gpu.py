"""GPU: de-emphasis through the streamed path.  With ``model.preemphasis = a`` ``WaveNet.generate_stream`` hands out the
PCM of ``ops.deemphasis_pcm16`` of ``generate()``'s classes -- the prompt's columns through the filter first, the state
carried over every chunk -- whatever the chunk size; with 0 it is the stream it was; and the sample logger's WAV files
hold the streamed bytes."""
import json
import wave
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import one_hot, synthetic_indices
from movenet_amd import ops
from movenet_amd.callbacks import LogSamplesCallback
from movenet_amd.generation import RingGenerator
from movenet_amd.utils.weights import make_state_dict
from movenet_amd.wavenet import WaveNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY = dict(layer_size=2, stack_size=2, input_channels=64, residual_channels=16, skip_channels=16)
Q, B, NEW, A = 64, 3, 300, 0.9


@pytest.fixture(scope="module")
def model():
    m = WaveNet(**TINY)
    m.load_state_dict(make_state_dict(**TINY, seed=3, gain=1.5, head_gain=6.0), strict=False)
    m = m.to(DEV).eval()
    m.generate_sampling = "model"
    m.generate_top_k, m.generate_top_p = 16, 0.9
    return m


def _prompt(m):
    return one_hot(synthetic_indices(B, m.receptive_fields, Q, 41), Q).to(DEV)


def _stream(m, a, chunk):
    m.preemphasis, m.generate_seed = a, 1234
    try:
        pieces = [(t0, pcm.copy()) for t0, pcm in m.generate_stream(_prompt(m), n_samples=m.receptive_fields + NEW,
                                                                    temperature=1.0, chunk=chunk)]
    finally:
        m.preemphasis = 0.0
    rf = m.receptive_fields
    assert [t0 for t0, _ in pieces] == [0] + [rf + k for k in range(0, NEW, chunk)]
    return np.concatenate([p for _, p in pieces], axis=1)


@pytest.fixture(scope="module")
def classes(model):
    """generate()'s classes under the stream's seed and settings -- generate() does not consult preemphasis"""
    model.generate_seed, model.preemphasis = 1234, A
    try:
        whole = model.generate(_prompt(model), n_samples=model.receptive_fields + NEW, temperature=1.0)
    finally:
        model.preemphasis = 0.0
    idx = whole.argmax(1).to(torch.int32).contiguous()
    assert len(torch.unique(idx[:, model.receptive_fields:])) > 8   # (the draws keep the clip moving)
    return idx


def test_stream_is_the_deemphasised_pcm_of_generates_classes_at_any_chunk(model, classes):
    want = ops.deemphasis_pcm16(classes, A, Q).cpu().numpy()
    assert not np.array_equal(want, ops.pcm16_chunk(classes, 0, classes.shape[1], Q).cpu().numpy())
    for chunk in (50, 300):
        got = _stream(model, A, chunk)
        assert got.dtype == np.int16 and got.shape == want.shape
        assert np.array_equal(got, want), (chunk, np.argwhere(got != want)[:5])


def test_without_preemphasis_the_stream_is_the_one_it_was(model, classes):
    want = ops.pcm16_chunk(classes, 0, classes.shape[1], Q).cpu().numpy()
    assert np.array_equal(_stream(model, 0.0, 50), want)


def test_ring_stream_carries_the_callers_state(model, classes):
    """RingGenerator.stream(deemphasis=a, state=...): the chunks continue a filter the caller has run over the prompt"""
    rf, n_total = model.receptive_fields, model.receptive_fields + NEW
    sd = {k: v for k, v in model._decoder_state().items() if ".context_conv_" not in k}
    g = RingGenerator(**TINY, state_dict=sd, batch=B, n_total=n_total, device=DEV, temperature=1.0, seed=1234,
                      sampling="model", top_k=16, top_p=0.9)
    g.prime(classes[:, :rf])
    state = torch.zeros(B, dtype=torch.float64, device=DEV)
    head = ops.pcm16_chunk(classes, 0, rf, Q, deemphasis=A, state=state).cpu().numpy()
    tail = np.concatenate([pcm.copy() for _, pcm in g.stream(NEW, 128, deemphasis=A, state=state)], axis=1)
    want = ops.deemphasis_pcm16(g.samples, A, Q).cpu().numpy()   # (whole clip, zero state: the generator's own classes)
    assert np.array_equal(np.concatenate([head, tail], axis=1), want)
    with pytest.raises(ValueError, match="state"):
        next(g.stream(1, 1, deemphasis=A, state=None))


def test_sample_logger_writes_the_streamed_bytes(model, classes, tmp_path):
    streamed = _stream(model, A, 50)
    rf = model.receptive_fields
    audio = one_hot(classes.cpu().to(torch.int64), Q).to(DEV)
    outputs = {"output": audio[:, :, rf:], "generated_output": audio}
    batch = (audio, None, ["tones"] * B, [f"clip{i}.wav" for i in range(B)], [{}] * B)
    trainer = SimpleNamespace(current_epoch=0, rank=0, root=None)
    module = SimpleNamespace(config=SimpleNamespace(model_config=SimpleNamespace(input_channels=Q)))
    LogSamplesCallback(log_every_n_epochs=1, out_dir=str(tmp_path), preemphasis=A).log_samples(
        "validation", trainer, module, outputs, batch, 0)
    rows = [json.loads(line) for line in open(tmp_path / "index.jsonl")]
    assert len(rows) == B and all(r["preemphasis"] == A for r in rows)
    for i, r in enumerate(rows):
        for key in ("gen_audio", "origin_audio"):
            with wave.open(str(tmp_path / r[key]), "rb") as w:
                assert (w.getnchannels(), w.getsampwidth()) == (1, 2)
                stored = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
            assert np.array_equal(stored, streamed[i]), (i, key)
    # off: the rows carry no such key and the files are the plain conversion
    LogSamplesCallback(log_every_n_epochs=1, out_dir=str(tmp_path / "off")).log_samples(
        "validation", trainer, module, outputs, batch, 0)
    rows = [json.loads(line) for line in open(tmp_path / "off" / "index.jsonl")]
    assert all("preemphasis" not in r for r in rows)
    with wave.open(str(tmp_path / "off" / rows[0]["gen_audio"]), "rb") as w:
        stored = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
    assert np.array_equal(stored, ops.pcm16_chunk(classes, 0, classes.shape[1], Q).cpu().numpy()[0])
