"""GPU: ``WaveNet.generate_stream(context="windowed")`` against ``context="whole"``, the PCM byte for byte
at the same chunking, on every kind of conditioning the windowed path takes; and the conditions of its design: a
windowed generator owns neither whole-context tensor, and its window buffers hold at most 2 x rows x chunk x C floats
however long the clip."""
import functools

import numpy as np
import pytest
import torch

from helpers import DEV, one_hot, synthetic_indices
from movenet_amd import _native as N
from movenet_amd import generation as G
from movenet_amd import ops
from movenet_amd import wavenet as W
from movenet_amd.utils.weights import make_state_dict
from movenet_amd.wavenet import WaveNet

pytestmark = pytest.mark.gpu

SMALL = dict(layer_size=3, stack_size=2, input_channels=64, residual_channels=16, skip_channels=8)     # GENERIC
C2 = dict(layer_size=10, stack_size=3, input_channels=256, residual_channels=64, skip_channels=64)     # FOLD under AUTO
N_NEW, HOP, MELS = 1200, 16, 8
CHUNKS = (1, 7, 1000)
# name -> (dims, batch, model keywords, labelled, guidance, groups forced, pre-emphasis)
SETUPS = {
    "mel":         (SMALL, 3, dict(local_channels=MELS, local_hop=HOP), False, 1.0, False, 0.0),
    "mel_window2": (SMALL, 3, dict(local_channels=MELS, local_hop=HOP, local_window=2), False, 1.0, False, 0.0),
    "label":       (C2, 2, dict(global_classes=3), True, 1.0, False, 0.0),
    "label_mel":   (SMALL, 3, dict(global_classes=3, local_channels=MELS, local_hop=HOP), True, 1.0, False, 0.0),
    "guided":      (C2, 2, dict(global_classes=3), True, 1.5, False, 0.0),
    "two_groups":  (C2, 2, dict(global_classes=3, local_channels=MELS, local_hop=HOP), True, 1.0, True, 0.0),
    "preemphasis": (SMALL, 3, dict(local_channels=MELS, local_hop=HOP), False, 1.0, False, 0.97),
}


@functools.lru_cache(maxsize=None)
def _model(name):
    cfg, _, extra, _, _, _, emph = SETUPS[name]
    torch.manual_seed(29)   # (global_embedding / local_conv keep their default initialisation, under this seed)
    m = WaveNet(**cfg, **extra)
    m.load_state_dict(make_state_dict(**cfg, seed=3, gain=1.5, head_gain=6.0), strict=False)
    m.preemphasis = emph
    return m.to(DEV).eval()


def _stream(name, chunk, context, monkeypatch, made=None):
    cfg, B, extra, labelled, guidance, grouped, _ = SETUPS[name]
    m = _model(name)
    Q, rf = cfg["input_channels"], m.receptive_fields
    n_total = rf + N_NEW
    m.generate_sampling, m.generate_top_k, m.generate_top_p, m.generate_seed = "model", 32, 0.9, 1234
    m.generate_guidance = guidance
    if "local_channels" in extra:
        g = torch.Generator().manual_seed(5)
        m.generate_local_features = torch.randn(B, MELS, (n_total - 1) // HOP + 1, generator=g).to(DEV)
    if grouped:  # two groups of one sequence each, taking turns on FOLD's pipelines
        monkeypatch.setattr(W, "auto_plan", lambda *a, **k: ("grouped", 1, N.GEN_FOLD))
    if made is not None:
        for cls in ("RingGenerator", "GroupedGenerator"):
            def record(*a, _cls=getattr(G, cls), **k):
                made.append(_cls(*a, **k))
                return made[-1]
            monkeypatch.setattr(W, cls, record)
    prompt = one_hot(synthetic_indices(B, rf, Q, 41), Q).to(DEV)
    labels = torch.tensor([2, 0, 1][:B]) if labelled else None
    try:
        pieces = [(t0, pcm.copy()) for t0, pcm in m.generate_stream(prompt, None, labels, n_samples=n_total,
                                                                    temperature=1.0, chunk=chunk, context=context)]
    finally:
        m.generate_guidance = 1.0
    assert m.last_generate_fallback is None
    return pieces, rf


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", list(SETUPS))
def test_windowed_stream_is_the_whole_context_stream_byte_for_byte(name, chunk, monkeypatch):
    cfg, B, extra, labelled, guidance, grouped, _ = SETUPS[name]
    want, rf = _stream(name, chunk, "whole", monkeypatch)
    made = []
    got, _ = _stream(name, chunk, "windowed", monkeypatch, made)
    assert [t0 for t0, _ in got] == [t0 for t0, _ in want] == [0] + list(range(rf, rf + N_NEW, chunk))
    for (t0, a), (_, b) in zip(got, want):
        assert a.dtype == np.int16 and a.shape == b.shape and a.tobytes() == b.tobytes(), (name, chunk, t0)
    if SETUPS[name][6] == 0.0:   # (under de-emphasis 0.97 the filtered PCM of these synthetic weights sits at the clip)
        assert len(np.unique(np.concatenate([p for _, p in want[1:]], axis=1))) > 1   # not one class repeated
    # the conditions of the design, on the generator(s) the windowed call built
    assert len(made) == 1 and isinstance(made[0], G.GroupedGenerator if grouped else G.RingGenerator)
    parts = made[0].groups if grouped else made
    assert len(parts) == (2 if grouped else 1)
    rows = sum(g.nrows for g in parts)
    assert rows == B * (2 if guidance != 1.0 else 1)
    for g in parts:
        assert g.context is None and g.context_tm is None
        assert g._source is not None and g._win is not None
    floats = sum(g._win.numel() for g in parts)
    assert floats <= 2 * rows * chunk * cfg["residual_channels"], (floats, rows, chunk)


def test_windowed_on_an_unconditioned_model_is_the_unconditioned_path(monkeypatch):
    cfg = SMALL
    m = WaveNet(**cfg)
    m.load_state_dict(make_state_dict(**cfg, seed=3, gain=1.5, head_gain=6.0), strict=False)
    m = m.to(DEV).eval()
    m.generate_sampling, m.generate_top_k, m.generate_top_p, m.generate_seed = "model", 32, 0.9, 7
    rf = m.receptive_fields
    prompt = one_hot(synthetic_indices(2, rf, 64, 41), 64).to(DEV)
    made = []

    def record(*a, **k):
        made.append(G.RingGenerator(*a, **k))
        return made[-1]
    monkeypatch.setattr(W, "RingGenerator", record)
    runs = {c: [p.copy() for _, p in m.generate_stream(prompt, n_samples=rf + 300, temperature=1.0, chunk=128, context=c)]
            for c in ("whole", "windowed")}
    assert all(np.array_equal(a, b) for a, b in zip(runs["whole"], runs["windowed"]))
    assert len(made) == 2 and all(g._source is None and g.context_tm is None for g in made)


def test_generator_argument_checks():
    cfg = SMALL
    sd = {k: v.to(DEV) for k, v in make_state_dict(**cfg, seed=3).items()}
    C = cfg["residual_channels"]
    glob = torch.zeros(2, C, device=DEV)
    src = G.ContextSource(glob=glob)
    kw = dict(state_dict=sd, batch=2, n_total=100, device=DEV)
    with pytest.raises(ValueError, match="one or the other"):
        G.RingGenerator(**cfg, **kw, context_source=src, global_context=glob)
    with pytest.raises(ValueError, match="one or the other"):
        G.RingGenerator(**cfg, **kw, context_source=src, context=torch.zeros(2, C, 100, device=DEV))
    with pytest.raises(ValueError, match="one or the other"):
        G.GroupedGenerator(**cfg, **kw, group=1, variant=N.GEN_GENERIC, context_source=src, global_context=glob)
    with pytest.raises(ValueError, match="context_source must hold"):
        G.RingGenerator(**cfg, **kw, context_source=G.ContextSource(glob=torch.zeros(3, C, device=DEV)))
    proj = torch.zeros(2, C, 5, device=DEV)
    with pytest.raises(ValueError, match="frames"):   # 5 frames at hop 16 reach column 79
        G.RingGenerator(**cfg, **kw, context_source=G.ContextSource(proj, 16, prompt=lambda P: None))
    with pytest.raises(ValueError, match="both None"):
        G.ContextSource()
    with pytest.raises(ValueError, match="prompt"):
        G.ContextSource(proj, 16)
    g = G.RingGenerator(**cfg, **kw, context_source=src)
    assert g.context is None and g.context_tm is None
    with pytest.raises(RuntimeError, match="whole-context"):
        g.teacher_forced(torch.zeros(2, 100, dtype=torch.int32, device=DEV), 0)
