"""Host: ``local_window`` / ``--mel_window`` where no GPU is needed -- the constructor's and
``set_local_conditioning``'s refusals, the k = 0 module being the module it was, the flag, the checkpoint record's default,
the resume check, the C entry points' refusals, and the float64 reference's own sanity."""
import pytest
import torch

import local_window_reference as W
import logmel_reference as R
from movenet_amd import _native as N
from movenet_amd import checkpoint
from movenet_amd.config import ModelConfig, TrainingConfig, arg_parser, config_from_args
from movenet_amd.wavenet import MAX_LOCAL_WINDOW, WaveNet

SHAPE = dict(layer_size=2, stack_size=2, input_channels=64, residual_channels=16, skip_channels=16)
SPEC = "synthetic://clips=6,frames=600,seed=5"


def test_constructor_and_set_local_conditioning_errors():
    assert MAX_LOCAL_WINDOW == 16
    for bad in (-1, 1.0, True, "2"):
        with pytest.raises(ValueError, match="local_window must be an integer >= 0"):
            WaveNet(**SHAPE, local_channels=8, local_hop=16, local_window=bad)
    with pytest.raises(ValueError, match="local_window must be at most 16, got 17"):
        WaveNet(**SHAPE, local_channels=8, local_hop=16, local_window=17)
    with pytest.raises(ValueError, match="needs local_channels"):
        WaveNet(**SHAPE, local_window=2)
    m = WaveNet(**SHAPE)
    with pytest.raises(ValueError, match="local_window must be an integer >= 0"):
        m.set_local_conditioning(8, 16, local_window=-2)
    with pytest.raises(ValueError, match="at most 16"):
        m.set_local_conditioning(8, 16, local_window=17)
    assert not hasattr(m, "local_conv")   # a refusal builds nothing
    m.set_local_conditioning(8, 16, local_window=16)
    assert m.local_conv.kernel_size == (33,) and m.local_window == 16
    conv = m.local_conv
    m.set_local_conditioning(8, 32, local_window=16)   # the same width and window: the conv stays, the hop moves
    assert m.local_conv is conv and m.local_hop == 32
    m.set_local_conditioning(8, 32)                     # back to the 1 x 1 conv
    assert m.local_conv.kernel_size == (1,) and m.local_window == 0
    # behind every other parameter, as before
    wide = WaveNet(**SHAPE, global_classes=3, local_channels=8, local_hop=16, local_window=2)
    assert list(wide.state_dict())[-2:] == ["local_conv.weight", "local_conv.bias"]
    assert tuple(wide.local_conv.weight.shape) == (16, 8, 5)


def test_window_zero_is_the_module_it_was():
    torch.manual_seed(11)
    a = WaveNet(**SHAPE, local_channels=8, local_hop=16)
    after_a = torch.rand(1)
    torch.manual_seed(11)
    b = WaveNet(**SHAPE, local_channels=8, local_hop=16, local_window=0)
    after_b = torch.rand(1)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)   # same keys, shapes, RNG draws
    assert torch.equal(after_a, after_b)
    assert tuple(sb["local_conv.weight"].shape) == (16, 8, 1) and b.local_window == 0
    # a window draws the other parameters as before: local_conv is registered last
    torch.manual_seed(11)
    c = WaveNet(**SHAPE, local_channels=8, local_hop=16, local_window=2)
    sc = c.state_dict()
    assert list(sc) == list(sa) and all(torch.equal(sa[k], sc[k]) for k in sa if not k.startswith("local_conv"))


def test_flag_and_config_field():
    base = ["--dataset", SPEC]
    assert config_from_args(arg_parser().parse_args(base)).mel_window == 0 and TrainingConfig().mel_window == 0
    cfg = config_from_args(arg_parser().parse_args(base + ["--use_mel", "1", "--use_video", "0", "--mel_window", "2"]))
    assert cfg.mel_window == 2 and cfg.use_mel
    assert TrainingConfig.from_json(cfg.to_json()).mel_window == 2
    with pytest.raises(ValueError, match="--mel_window 2 needs --use_mel 1"):
        config_from_args(arg_parser().parse_args(base + ["--mel_window", "2"]))
    for bad in ("-1", "17"):
        with pytest.raises(ValueError, match="--mel_window must lie in"):
            config_from_args(arg_parser().parse_args(base + ["--use_mel", "1", "--mel_window", bad]))


def _module(tmp_path, **over):
    from movenet_amd.pytorch_lightning_trainer import Dance2Music
    kw = dict(model_config=ModelConfig(**SHAPE), batch_size=2, val_batch_size=2, n_epochs=2, use_video=False,
              use_mel=True, mel_bins=8, mel_fft=64, mel_hop=16, optimizer="AdamW", scheduler=None,
              model_output_path=tmp_path / "run")
    return Dance2Music(SPEC, TrainingConfig(**{**kw, **over}))


def _written(tmp_path, module, name):
    """A checkpoint of one CPU step of ``module``, through the writer the trainer uses."""
    opt = module.configure_optimizers()["optimizer"]
    for p in module.model.parameters():
        p.grad = torch.full_like(p, 0.01)
    opt.step()
    obj = checkpoint.training_checkpoint(module, opt, None, epoch=0, global_step=3, next_epoch=1, batches_done=0,
                                         hyper=checkpoint.hyper_parameters(module.config, SPEC), history_len=3)
    checkpoint.write_checkpoint(obj, tmp_path / name)
    return tmp_path / name


def test_module_builds_the_windowed_conv_and_the_record_carries_the_key_only_then(tmp_path):
    from movenet_amd.pytorch_lightning_trainer import Dance2Music
    plain, wide = _module(tmp_path), _module(tmp_path, mel_window=2)
    assert plain.model.local_conv.kernel_size == (1,) and wide.model.local_conv.kernel_size == (5,)
    assert "local_window" not in plain.local_conditioning and "local_window" not in plain.model.local_conditioning
    assert wide.local_conditioning["local_window"] == 2 and wide.model.local_conditioning["local_window"] == 2
    with pytest.raises(ValueError, match="--mel_window 2 needs --use_mel 1"):
        Dance2Music(SPEC, TrainingConfig(model_config=ModelConfig(**SHAPE), use_video=False, mel_window=2))
    p0, p2 = _written(tmp_path, plain, "plain.ckpt"), _written(tmp_path, wide, "wide.ckpt")
    rec0, rec2 = checkpoint.local_conditioning_of(p0), checkpoint.local_conditioning_of(p2)
    assert set(rec0) == {"local_channels", "local_hop", "mel_fft", "mel_fmin", "mel_fmax", "audio_rate"}
    assert rec2 == {**rec0, "local_window": 2}
    # readers: a record without the key is window 0
    assert checkpoint.local_window_of(rec0) == 0 and checkpoint.local_window_of(rec2) == 2
    assert checkpoint.local_window_of(None) == 0
    a, b = WaveNet(**SHAPE), WaveNet(**SHAPE)
    checkpoint.load_into(a, p0)
    checkpoint.load_into(b, p2)
    assert (a.local_window, a.local_conv.kernel_size) == (0, (1,))
    assert (b.local_window, b.local_conv.kernel_size) == (2, (5,))
    assert torch.equal(b.local_conv.weight, wide.model.local_conv.weight)


def test_synthesize_load_model_reads_the_window(tmp_path):
    from types import SimpleNamespace

    from movenet_amd.synthesize import load_model

    def fail(message):
        raise AssertionError(message)
    for window, taps in ((0, 1), (2, 5)):
        path = _written(tmp_path, _module(tmp_path, mel_window=window), f"w{window}.ckpt")
        args = SimpleNamespace(checkpoint=str(path), ema=0, preemphasis=None, force_preemphasis=0, **{k: None for k in SHAPE})
        model, rec, _ = load_model(args, fail)
        assert model.local_window == window and model.local_conv.kernel_size == (taps,)
        assert ("local_window" in rec) == (window > 0)


@pytest.mark.parametrize("saved,run", [(0, 2), (2, 0), (2, 3)])
def test_resume_under_another_window_is_refused_before_the_gpu(tmp_path, saved, run):
    from movenet_amd.pytorch_lightning_trainer import Trainer
    path = _written(tmp_path, _module(tmp_path, mel_window=saved), "last.ckpt")
    trainer = Trainer(max_epochs=2, default_root_dir=tmp_path / "run", device="cpu")
    with pytest.raises(ValueError) as e:
        trainer.fit(_module(tmp_path, mel_window=run), ckpt_path=path)
    assert str(path) in str(e.value) and "local_conditioning['local_window']" in str(e.value)
    assert f"is {saved}, but this run has {run}" in str(e.value)


def test_entry_points_are_declared_and_refuse_bad_taps_without_a_gpu():
    assert "mvn_upsample_features_win" in N.SIGNATURES and "mvn_upsample_features_win_backward" in N.SIGNATURES
    lib = N.lib()
    p = 256   # (never dereferenced: every call below is refused, or returns, before a launch)
    for taps in (0, 2, 4, 35, -1):
        rc = lib.mvn_upsample_features_win(p, 8, p, p, 1, 4, 8, 4, taps, 16, 100, p, 100, p, 32, None)
        assert rc == N.MVN_ERR_BAD_ARG and "taps" in N.last_error(), taps
        rc = lib.mvn_upsample_features_win_backward(p, 100, p, 8, p, 1, 4, 8, 4, taps, 16, 100, p, p, p, 8, p, 32, None)
        assert rc == N.MVN_ERR_BAD_ARG and "taps" in N.last_error(), taps
    assert lib.mvn_upsample_features_win(p, 8, p, p, 1, 4, 6, 4, 3, 16, 100, p, 100, p, 32, None) == N.MVN_ERR_BAD_ARG
    assert "too few frames" in N.last_error()
    assert lib.mvn_upsample_features_win(p, 8, p, p, 1, 4, 8, 4, 3, 16, 100, p, 102, p, 32, None) == N.MVN_ERR_BAD_ARG
    assert "multiple of 4" in N.last_error()
    assert lib.mvn_upsample_features_win(p, 8, p, p, 1, 4, 8, 4, 3, 16, 100, p, 100, p, 31, None) == N.MVN_ERR_BAD_ARG
    assert "scratch" in N.last_error()
    assert lib.mvn_upsample_features_win(p, 8, p, p, 0, 4, 8, 4, 33, 16, 100, p, 100, p, 0, None) == N.MVN_OK
    assert lib.mvn_upsample_features_win_backward(p, 100, p, 8, p, 0, 4, 8, 4, 33, 16, 100, p, p, p, 8, p, 0,
                                                  None) == N.MVN_OK


# ---- the float64 reference's own sanity ----
def _data(B, M, F, C, hop, T, k, seed=3):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, M, F, generator=g, dtype=torch.float64),
            torch.randn(C, M, 2 * k + 1, generator=g, dtype=torch.float64),
            torch.randn(C, generator=g, dtype=torch.float64), torch.randn(B, C, T, generator=g, dtype=torch.float64))


def test_reference_without_a_window_is_the_existing_reference():
    mel, w, bias, _ = _data(2, 5, 7, 6, 16, 100, 0)
    got = W.upsample_features_win(mel, w, bias, 16, 100)
    want = R.upsample_features(mel, w[:, :, 0], bias, 16, 100)
    assert float((got - want).abs().max()) < 1e-13 * float(want.abs().max())


@pytest.mark.parametrize("shape", [(2, 5, 7, 6, 16, 100, 2), (2, 3, 3, 4, 4, 9, 4), (1, 4, 1, 4, 16, 16, 2)])
def test_reference_follows_the_clamped_definition_and_the_dmel_edge_identity(shape):
    B, M, F, C, hop, T, k = shape
    mel, w, bias, dctx = _data(*shape)
    ref = W.reference(mel, w, bias, dctx, hop, T)
    # the definition, index by index: cl(j + d) = min(max(j + d, 0), F - 1)
    proj = bias[None, :, None].expand(B, C, F).clone()
    for j in range(F):
        for d in range(-k, k + 1):
            proj[:, :, j] += torch.einsum("cm,bm->bc", w[:, :, d + k], mel[:, :, min(max(j + d, 0), F - 1)])
    assert float((W.project(mel, w, bias) - proj).abs().max()) < 1e-12
    # every (j, d) pair lands on exactly one frame, so the frames of dmel sum to sum_{c, d} w dP summed over j
    dP = W.frame_gradient(dctx, F, hop)
    want = torch.einsum("cm,bc->bm", w.sum(2), dP.sum(2))
    got = ref["dmel"].sum(2)
    assert float((got - want).abs().max()) < 1e-12 * max(1.0, float(want.abs().max()))
    # and the edge frames hold what the header says: frame 0 every j <= -d, frame F - 1 every j >= F - 1 - d
    first, last = torch.zeros(B, M, dtype=torch.float64), torch.zeros(B, M, dtype=torch.float64)
    for d in range(-k, k + 1):
        for j in range(F):
            term = torch.einsum("cm,bc->bm", w[:, :, d + k], dP[:, :, j])
            if min(max(j + d, 0), F - 1) == 0:
                first += term
            if min(max(j + d, 0), F - 1) == F - 1:
                last += term
    assert float((ref["dmel"][:, :, 0] - first).abs().max()) < 1e-12 * max(1.0, float(first.abs().max()))
    assert float((ref["dmel"][:, :, -1] - last).abs().max()) < 1e-12 * max(1.0, float(last.abs().max()))
