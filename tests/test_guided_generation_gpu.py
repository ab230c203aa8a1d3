"""GPU: classifier-free guidance (mvn_generate_guided, include/movenet_hip.h) on every kernel that has a
guided form -- GENERIC, PIPE, FOLD, PIPE_F16.  Every case starts from a zero state with a one-sample prompt (or, through
WaveNet.generate, a receptive field of prompt) and runs N_STEPS steps.

Pairs per launch: 1, 3, 4 and the variant's limit for the dims (mvn_gen_guided_max_pairs) -- on the two short models
q64 and q128, whose pipelines are two and three stages long (FOLD: 128 of them), the limit is capped at MAXP = 24; the
true limits, cross-XCD pipelines included, run on c2 (FOLD 23, PIPE 24) and wide (PIPE 4, PIPE_F16 8).

q64 is 3 x 2 layers: FOLD packs three layers per stage, and a model whose layer count is no multiple of three ends in
a stage padded with zero layers.  The UNGUIDED FOLD launch of such a model (4 x 1 layers, 16 sequences or more, this
change's parent included) was seen to return NaN logits in some rows from run to run; the cases here, which compare
guided launches with unguided ones bit by bit, stay off that form."""
import functools

import numpy as np
import pytest
import torch

import guided_reference as GR
import sampling_reference as R
import test_truncated_sampling_gpu as T
from movenet_amd import _native as N
from movenet_amd.generation import GroupedGenerator, RingGenerator
from movenet_amd.utils.weights import make_state_dict, one_hot, synthetic_indices
from oracle import wavenet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_STEPS = 64
MAXP = 24  # the most pairs any case launches (PIPE at config 2)


def _cfg(layer_size, stack_size, Q, C, K):
    return dict(layer_size=layer_size, stack_size=stack_size, input_channels=Q, residual_channels=C, skip_channels=K)


SHAPES = {"small": _cfg(2, 2, 64, 16, 16), "c2": _cfg(10, 3, 256, 64, 64), "wide": _cfg(10, 6, 256, 128, 128),
          "q64": _cfg(3, 2, 64, 64, 64), "q128": _cfg(4, 1, 128, 64, 64)}
VARIANTS = {"GENERIC": N.GEN_GENERIC, "PIPE": N.GEN_PIPE, "FOLD": N.GEN_FOLD, "PIPE_F16": N.GEN_PIPE_F16}
CASES = [("GENERIC", "small"), ("GENERIC", "c2"), ("PIPE", "c2"), ("FOLD", "c2"), ("PIPE", "wide"), ("PIPE_F16", "wide"),
         ("FOLD", "q64"), ("PIPE", "q128")]
IDS = [f"{v}-{s}" for v, s in CASES]
SCALES = [0.0, 0.5, 3.0, -1.0]
SAMPLED = (1.0, 40, 0.9)  # temperature, top_k, top_p of the sampled cases


@functools.lru_cache(maxsize=None)
def _weights(shape):
    return {k: v.to(DEV) for k, v in make_state_dict(**SHAPES[shape], seed=3, gain=1.5, head_gain=6.0).items()}


@functools.lru_cache(maxsize=None)
def _label_vectors(shape, pairs):
    g = torch.Generator().manual_seed(17)
    return torch.randn(pairs, SHAPES[shape]["residual_channels"], generator=g).to(DEV)


def _limit(variant, shape):
    return min(int(N.guided_max_pairs(N.make_dims(**SHAPES[shape]), VARIANTS[variant])), MAXP)


def _settings(pairs, sampled, seed0=100):
    t, k, p = SAMPLED if sampled else (0.0, 0, 1.0)
    return dict(temperature=[t] * pairs, top_k=[k] * pairs, top_p=[p] * pairs, seed=[seed0 + b for b in range(pairs)])


def _guided(variant, shape, pairs, scales, sampled, sampling="model", rows=None, first=0, n_total=N_STEPS + 1):
    """A guided generator of pairs [first, first + pairs) of the shape's label vectors."""
    vec = _label_vectors(shape, MAXP)[first:first + pairs]
    s = _settings(MAXP, sampled)
    s = {k: v[first:first + pairs] for k, v in s.items()}
    return RingGenerator(**SHAPES[shape], state_dict=_weights(shape), batch=pairs, n_total=n_total, device=DEV,
                         variant=VARIANTS[variant], sampling=sampling, global_context=vec, guidance=scales,
                         rows=list(range(first, first + pairs)) if rows is None else rows, **s)


def _unguided_rows(variant, shape, pairs, sampled, sampling="model", both=True, n_total=N_STEPS + 1):
    """The same rows in an unguided mvn_generate_seq launch: contexts 0 (``both``) and e, the pairs' settings and rows."""
    vec = _label_vectors(shape, MAXP)[:pairs]
    s = {k: v[:pairs] * (2 if both else 1) for k, v in _settings(MAXP, sampled).items()}
    ctx = torch.cat([torch.zeros_like(vec), vec], 0) if both else vec
    rows = list(range(pairs)) * (2 if both else 1)
    # PIPE_F16 folds three layers into a stage where every pipeline serves one sequence and two where they serve
    # several (as a guided launch's do): other sums, other bits.  Like is compared with like: rows that repeat row 0
    # are appended until the unguided launch runs the several-sequences form too (callers index the rows they mean).
    pipes = N.lib().mvn_gen_launch_pipelines(N.make_dims(**SHAPES[shape]), VARIANTS[variant], 1 << 20)
    extra = max(0, pipes + 1 - len(rows)) if variant == "PIPE_F16" else 0
    if extra:
        ctx = torch.cat([ctx, ctx[:1].repeat(extra, 1)], 0)
        s = {k: v + v[:1] * extra for k, v in s.items()}
        rows = rows + rows[:1] * extra
    return RingGenerator(**SHAPES[shape], state_dict=_weights(shape), batch=len(ctx), n_total=n_total, device=DEV,
                         variant=VARIANTS[variant], sampling=sampling, global_context=ctx, rows=rows, **s)


def _history(shape, B, seed=4321):
    return synthetic_indices(B, N_STEPS + 1, SHAPES[shape]["input_channels"], seed).to(DEV)


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _free_run(g, prompt, parts=(N_STEPS,), out=False):
    """Free run from a one-sample prompt; ``out``: also the launch's choices_out / logits_out of all rows."""
    g.prime(prompt)
    logits = choices = None
    if out:
        logits = torch.zeros(g.nrows, g.n_total - 1, g.Q, dtype=torch.float32, device=DEV)
        choices = torch.full((g.nrows, g.n_total), -1, dtype=torch.int32, device=DEV)
        g._run(0, g.n_total - 1, 1, logits, choices, 1)
        g.t = g.n_total - 1
    else:
        for n in parts:
            g.advance(n)
    g.check_errors()
    return g.samples_all.clone(), choices, logits


# ---- 1. s = 1 is conditional generation, to the bit ---------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", CASES, ids=IDS)
@pytest.mark.parametrize("sampling", ["model", "reference"])
def test_scale_one_is_conditional_generation_to_the_bit(variant, shape, sampling):
    pairs = _limit(variant, shape)
    prompt = _history(shape, pairs, seed=99)[:, :1]
    g = _guided(variant, shape, pairs, 1.0, True, sampling)
    samples, choices, logits = _free_run(g, prompt, out=True)
    u = _unguided_rows(variant, shape, pairs, True, sampling, both=False)
    want, want_choices, want_logits = (x[:pairs] for x in _free_run(u, prompt[list(range(pairs)) + [0] * (u.batch - pairs)],
                                                                  out=True))
    bad = (samples[pairs:] != want).nonzero()
    same_logits = (logits[pairs:] == want_logits).all(-1)
    print(f"{variant} {shape} {sampling}: {pairs} pairs; samples differ at {len(bad)} places, first {bad[:3].tolist()}; "
          f"logits rows that differ: {(~same_logits).nonzero()[:3].tolist()} of {int((~same_logits).sum())}")
    assert torch.equal(samples[pairs:], want) and torch.equal(samples[:pairs], want)
    assert torch.equal(choices[pairs:], want_choices) and torch.equal(choices[:pairs], want_choices)
    assert np.array_equal(_bits(logits[pairs:]), _bits(want_logits))
    assert len(torch.unique(want[:, 1:])) > 1


# ---- 2. combine and choice, every kernel --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _unguided_teacher_forced(variant, shape):
    """Raw logits of the rows of test 2 (4 pairs: contexts 0 | e) from the unguided teacher-forced launch; shared."""
    u = _unguided_rows(variant, shape, 4, False)
    hist = _history(shape, 4)
    _, logits = u.teacher_forced(torch.cat([hist, hist, hist[:1].repeat(u.batch - 8, 1)], 0), logits_t0=1)
    u.check_errors()
    return logits[:8].cpu().numpy()


@pytest.mark.parametrize("variant,shape", CASES, ids=IDS)
@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_combine_and_choice(variant, shape, sampled):
    pairs, Q = 4, SHAPES[shape]["input_channels"]
    g = _guided(variant, shape, pairs, SCALES, sampled)
    g.teacher_forced(_history(shape, pairs), logits_t0=1)
    g.check_errors()
    choices, logits = (x.cpu().numpy() for x in g.teacher_forced_all)
    raw = _unguided_teacher_forced(variant, shape)
    assert np.array_equal(logits.view(np.uint32), raw.view(np.uint32))  # each row's own raw logits
    assert np.array_equal(choices[:pairs], choices[pairs:]) and (choices[:, 0] == -1).all()
    lg = GR.guided_logits(logits[pairs:], logits[:pairs], np.array(SCALES)[:, None])
    assert lg.shape == (pairs, N_STEPS, Q) and np.isfinite(lg).all()
    picks = choices[pairs:, 1:]
    assert picks.min() >= 0 and picks.max() < Q
    if not sampled:
        clear = GR.top2_margin(lg) >= 1e-3
        print(f"{variant} {shape}: {(~clear).sum()} of {clear.size} steps with a top-2 margin below 1e-3")
        assert np.array_equal(picks[clear], lg.argmax(-1)[clear])
        assert np.array_equal(picks[~clear], GR.greedy_picks(lg)[~clear])
        return
    t, k, p = SAMPLED
    for b in range(pairs):  # (top_k < Q on every shape)
        uniform = R.philox_uniform(100 + b, np.arange(1, N_STEPS + 1)[None, :], np.array([[b]]))
        T._check_truncated_draws(picks[b:b + 1], lg[b:b + 1], t, k, p, uniform, Q, f"{variant} {shape} s={SCALES[b]}")


# ---- 3. the pick reaches both rows ------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", CASES, ids=IDS)
def test_the_pick_reaches_both_rows(variant, shape):
    pairs, scales = 3, [3.0, 0.5, -1.0]
    prompt = _history(shape, pairs, seed=99)[:, :1]
    g = _guided(variant, shape, pairs, scales, True)
    S, choices, logits = _free_run(g, prompt, out=True)
    assert torch.equal(S[:pairs], S[pairs:]) and torch.equal(choices[:, 1:], S[:, 1:])
    assert len(torch.unique(S[:, 1:])) > 1
    g.teacher_forced(S[pairs:], logits_t0=1)
    g.check_errors()
    again, again_logits = g.teacher_forced_all
    assert torch.equal(again[:, 1:], S[:, 1:])
    assert np.array_equal(_bits(again_logits), _bits(logits))
    assert not np.array_equal(_bits(logits[:pairs]), _bits(logits[pairs:]))


# ---- 4. against the oracle, small dims --------------------------------------------------------------------------------
def test_greedy_guided_generation_equals_the_reference():
    cfg, pairs, s = SHAPES["small"], 2, 3.0
    sd = make_state_dict(**cfg, seed=3, gain=1.5, head_gain=6.0)
    vec = _label_vectors("small", MAXP)[:pairs]
    prompt = _history("small", pairs, seed=99)[:, :1]
    want, _, _, lg = GR.generate_guided(sd, O.Dims(**cfg), prompt.cpu().numpy(), N_STEPS + 1, vec.cpu().numpy(), s)
    margin = GR.top2_margin(lg[:, 1:])
    print(f"reference's smallest guided top-2 margin over {margin.size} steps: {margin.min():.4g}")
    assert margin.min() >= 1e-3  # no step is excused
    g = RingGenerator(**cfg, state_dict=_weights("small"), batch=pairs, n_total=N_STEPS + 1, device=DEV,
                      variant=N.GEN_GENERIC, global_context=vec, guidance=s)
    S, _, _ = _free_run(g, prompt)
    assert np.array_equal(S[pairs:].cpu().numpy(), want) and np.array_equal(S[:pairs].cpu().numpy(), want)
    assert len(np.unique(want[:, 1:])) > 1


# ---- 5. independence and chunking -------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", CASES, ids=IDS)
def test_pairs_are_independent_and_chunks_add_up(variant, shape):
    pairs, scales = 3, [3.0, 0.5, -1.0]
    prompt = _history(shape, pairs, seed=99)[:, :1]
    together, _, _ = _free_run(_guided(variant, shape, pairs, scales, True), prompt)
    for p in range(pairs):
        alone, _, _ = _free_run(_guided(variant, shape, 1, [scales[p]], True, first=p), prompt[p:p + 1])
        assert torch.equal(alone[1], together[pairs + p]) and torch.equal(alone[0], together[p]), p
    assert not torch.equal(together[pairs], together[pairs + 1])
    chunked, _, _ = _free_run(_guided(variant, shape, pairs, scales, True), prompt, parts=(13, N_STEPS - 13))
    assert torch.equal(chunked, together)


def test_grouped_generator_groups_by_pairs():
    pairs, scales = 5, [3.0, 0.5, -1.0, 2.0, 0.0]
    prompt = _history("c2", pairs, seed=99)[:, :1]
    s = _settings(pairs, True)
    vec = _label_vectors("c2", MAXP)[:pairs]
    kw = dict(state_dict=_weights("c2"), batch=pairs, n_total=N_STEPS + 1, device=DEV, variant=N.GEN_FOLD,
              sampling="model", global_context=vec, guidance=scales, **s)
    single, _, _ = _free_run(RingGenerator(**SHAPES["c2"], **kw), prompt)
    gg = GroupedGenerator(**SHAPES["c2"], group=2, **kw)
    assert gg.bounds == [(0, 2), (2, 4), (4, 5)] and [g.nrows for g in gg.groups] == [4, 4, 2]
    gg.prime(prompt)
    gg.advance(N_STEPS)
    gg.check_errors()
    assert torch.equal(gg.samples, single[pairs:])


# ---- 6. refusals with a device; guard bands ---------------------------------------------------------------------------
def test_refusals_touch_nothing():
    g = _guided("FOLD", "c2", 2, 2.0, False)
    before = (g.state.clone(), g.samples_all.clone())
    lib, dims = N.lib(), N.make_dims(**SHAPES["c2"])

    def call(variant, pairs, per_seq=True, guidance=True):
        return lib.mvn_generate_guided(dims, variant, g.packed.data_ptr(), g.state.data_ptr(), g.samples_all.data_ptr(),
                                       pairs, g.n_total, g.n_total, 1, 0, 8, g._per_seq.data_ptr() if per_seq else None,
                                       g._guidance.data_ptr() if guidance else None, None, None, 0,
                                       g.context_tm.data_ptr(), N.SAMPLE_MODEL, None)
    assert call(N.GEN_FOLD, 24) == N.MVN_ERR_UNSUPPORTED and "at most 23 pairs" in N.last_error()
    assert call(N.GEN_STREAM, 2) == N.MVN_ERR_UNSUPPORTED and "at most 0 pairs" in N.last_error()
    assert call(N.GEN_FOLD, 2, per_seq=False) == N.MVN_ERR_BAD_ARG
    assert call(N.GEN_FOLD, 2, guidance=False) == N.MVN_ERR_BAD_ARG
    assert call(N.GEN_FOLD, 0) == N.MVN_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert torch.equal(g.state, before[0]) and torch.equal(g.samples_all, before[1])
    with pytest.raises(RuntimeError, match="at most 23 pairs"):
        _guided("FOLD", "c2", 24, 2.0, False)
    with pytest.raises(RuntimeError):
        RingGenerator(**SHAPES["c2"], state_dict=_weights("c2"), batch=2, n_total=9, device=DEV, variant=N.GEN_STREAM,
                      global_context=_label_vectors("c2", MAXP)[:2], guidance=2.0)


def test_guard_bands_stay_intact(monkeypatch):
    monkeypatch.setenv("MOVENET_DEBUG_GUARD", "1")
    for variant, shape in CASES:
        pairs = _limit(variant, shape)
        g = _guided(variant, shape, pairs, [SCALES[p % 4] for p in range(pairs)], True)
        assert g._guard is not None
        S, _, _ = _free_run(g, _history(shape, pairs, seed=99)[:, :1])  # (check_errors compares the bands)
        assert int(S.min()) >= 0 and int(S.max()) < SHAPES[shape]["input_channels"]


# ---- 7. WaveNet.generate ----------------------------------------------------------------------------------------------
def test_wavenet_generate_with_guidance():
    from movenet_amd.wavenet import WaveNet
    cfg, G, B, n_new = SHAPES["small"], 3, 3, N_STEPS
    dims = O.Dims(**cfg)
    rf = dims.receptive_fields
    torch.manual_seed(11)
    model = WaveNet(**cfg, global_classes=G)
    sd = make_state_dict(**cfg, seed=3, gain=1.5, head_gain=6.0)
    model.load_state_dict(sd, strict=False)
    model.to(DEV)
    labels = torch.tensor([2, 0, 1])
    prompt_idx = synthetic_indices(B, rf, 64, 11)
    prompt = one_hot(prompt_idx, 64).to(DEV)
    plain = model.generate(prompt, None, labels, n_samples=rf + n_new, temperature=0.0)
    model.generate_guidance = 1.0
    assert torch.equal(model.generate(prompt, None, labels, n_samples=rf + n_new, temperature=0.0), plain)
    e = model.global_embedding.weight.detach()[labels].cpu().numpy()
    full = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    want, _, _, lg = GR.generate_guided(full, dims, prompt_idx.numpy(), rf + n_new, e, 3.0)
    margin = GR.top2_margin(lg[:, rf:])
    print(f"reference's smallest guided top-2 margin: {margin.min():.4g}")
    assert margin.min() >= 1e-3
    model.generate_guidance = 3.0
    out = model.generate(prompt, None, labels, n_samples=rf + n_new, temperature=0.0)
    assert np.array_equal(out.argmax(1).cpu().numpy(), want)
    assert not torch.equal(out, plain)
    # a list of scales equals the scalar runs
    model.generate_guidance = [3.0, 1.0, 0.0]
    mixed = model.generate(prompt, None, labels, n_samples=rf + n_new, temperature=0.0)
    model.generate_guidance = 0.0
    zero = model.generate(prompt, None, labels, n_samples=rf + n_new, temperature=0.0)
    assert torch.equal(mixed[0], out[0]) and torch.equal(mixed[1], plain[1]) and torch.equal(mixed[2], zero[2])


def test_a_dropped_label_reaches_the_kernels_as_the_zero_vector():
    """Train-mode forward with P = 1 is forward with e = 0 (all-zero mixture rows), to the bit; eval mode never drops.
    q64: C = K = 64, the fast path of global conditioning; small: the context path."""
    from movenet_amd.wavenet import WaveNet
    for shape in ("small", "q64"):
        cfg, B, G = SHAPES[shape], 3, 4
        torch.manual_seed(3)
        model = WaveNet(**cfg, global_classes=G)
        model.load_state_dict(make_state_dict(**cfg, seed=3, gain=1.5), strict=False)
        model.to(DEV)
        x = one_hot(synthetic_indices(B, 120, cfg["input_channels"], 5), cfg["input_channels"]).to(DEV)
        labels = torch.tensor([1, 3, 0])
        model.eval()
        with torch.no_grad():
            labelled = model(x, None, labels)
            unlabelled = model(x, None, torch.zeros(B, G))
            model.global_dropout = 1.0
            assert torch.equal(model(x, None, labels), labelled)       # eval: no dropout
            model.train()
            assert torch.equal(model(x, None, labels), unlabelled)     # train, P = 1: every row is e = 0
            model.global_dropout = 0.0
            assert torch.equal(model(x, None, labels), labelled)
        assert not torch.equal(labelled, unlabelled)
        # a partial mask: the dropped rows are the unlabelled rows, the kept ones the labelled rows
        model.global_dropout = 0.5
        model.global_dropout_generator = torch.Generator().manual_seed(1)
        keep = (torch.rand(B, generator=torch.Generator().manual_seed(1)) >= 0.5)
        assert 0 < int(keep.sum()) < B
        with torch.no_grad():
            mixed = model(x, None, labels)
        for b in range(B):
            assert torch.equal(mixed[b], (labelled if keep[b] else unlabelled)[b]), (shape, b)


# ---- 8. trainer -----------------------------------------------------------------------------------------------------------
def test_trainer_with_label_dropout_and_guided_samples(tmp_path):
    import json
    from movenet_amd.config import arg_parser, config_from_args
    from movenet_amd.pytorch_lightning_trainer import Dance2Music, Trainer
    out = tmp_path / "run"
    spec = "synthetic://clips=4,frames=60,seed=2"
    args = arg_parser().parse_args([
        "--dataset", spec, "--use_video", "0", "--use_global", "1", "--global_dropout", "0.5", "--generate_guidance", "2",
        "--log_samples_every", "1", "--input_channels", "64", "--residual_channels", "16", "--skip_channels", "16",
        "--layer_size", "2", "--stack_size", "2", "--batch_size", "2", "--val_batch_size", "2", "--n_epochs", "1",
        "--num_workers", "0", "--val_num_workers", "0", "--model_output_path", str(out)])
    torch.manual_seed(5)
    module = Dance2Music(spec, config_from_args(args))
    assert module.model.global_dropout == 0.5 and module.model.generate_guidance == 2.0
    from movenet_amd.callbacks import LogSamplesCallback
    trainer = Trainer(max_epochs=1, default_root_dir=str(out),
                      callbacks=[LogSamplesCallback(log_every_n_epochs=1, guidance=2.0)])
    gen = module.model.global_dropout_generator
    moved = {"train": [], "val": []}  # per step: did the dropout generator's state move?

    def watched(step, kind):
        def run(batch, batch_idx):
            before = gen.get_state()
            out = step(batch, batch_idx)
            moved[kind].append(not torch.equal(gen.get_state(), before))
            return out
        return run
    module.training_step = watched(module.training_step, "train")
    module.validation_step = watched(module.validation_step, "val")
    trainer.fit(module)
    assert trainer.history and all(np.isfinite(r["train_loss"]) for r in trainer.history)
    # every train step draws a mask -- the ones behind a logged sample too, whose generate() left the model in eval
    # mode -- and no validation step, nor the generate() calls inside either, touches the generator
    assert len(moved["train"]) >= 2 and all(moved["train"]), moved
    assert moved["val"] and not any(moved["val"]), moved
    rows = [json.loads(line) for line in open(out / "samples" / "index.jsonl")]
    assert rows and all(r["guidance"] == 2.0 and "gen_audio" in r for r in rows)
