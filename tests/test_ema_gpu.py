"""GPU: the exponential moving average (EMA) of the weights kept by the fused AdamW step.

1. ``mvn_adamw_ema_step`` through the raw C ABI: ``p``, ``m``, ``v`` bit-equal to ``mvn_adamw_step``'s, the average
   against a float64 recurrence, skipped elements and a guard band behind every buffer untouched.
2. ``FlatAdamW(ema_decay=...)`` against torch's optimizer and a float64 average of torch's parameters.
3. ``averaged_parameters()``: a swap of views, no copy, safe against exceptions and misuse.
4. ``state_dict`` / ``load_state_dict`` carry the average.
5. The trainer validates, samples and checkpoints with the averaged weights.

The bound on the average (tests 1 and 2).  One update ``e + (p - e) w`` rounds three times: the difference (at most
2M in magnitude, M the largest |p| or |e| seen: an error of at most 2^-24 . 2M, which w <= 1 does not enlarge), the
product (at most 2M again: 2^-24 . 2M) and the sum (at most M: 2^-24 . M) -- 2^-24 . 5M together.  An error already in
``e`` is multiplied by ``1 - w = decay_t <= decay`` per update, so the errors sum to at most
5 . 2^-24 . M / (1 - decay)."""
import copy
import ctypes
from dataclasses import asdict

import numpy as np
import pytest
import torch

from helpers import one_hot, rel_err, synthetic_indices
from movenet_amd import _native as N
from movenet_amd.utils.weights import make_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DECAY = 0.9
HYPER = dict(lr=3e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.05)


def _ema_bound(big: float) -> float:
    return 5.0 * 2.0 ** -24 * big / (1.0 - DECAY)


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _skips(ranges):
    return (ctypes.c_size_t * max(2 * len(ranges), 1))(*[x for r in ranges for x in r]), len(ranges)


def _plain_step(p, g, m, v, n, step, decoupled, ranges):
    arr, k = _skips(ranges)
    h = HYPER
    rc = N.lib().mvn_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, h["lr"], h["beta1"],
                                h["beta2"], h["eps"], h["wd"], step, decoupled, arr, k, _stream())
    assert rc == N.MVN_OK, N.last_error()


def _ema_step(p, g, m, v, e, n, step, decoupled, w, ranges):
    arr, k = _skips(ranges)
    h = HYPER
    rc = N.lib().mvn_adamw_ema_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), e.data_ptr(), n,
                                    h["lr"], h["beta1"], h["beta2"], h["eps"], h["wd"], step, decoupled, w, arr, k,
                                    _stream())
    assert rc == N.MVN_OK, N.last_error()


# ---- 1. the kernel, raw C ABI -------------------------------------------------------------------------------------
@pytest.mark.parametrize("warmup", [True, False], ids=["warmup", "constant"])
@pytest.mark.parametrize("decoupled", [1, 0], ids=["adamw", "adam"])
def test_kernel_against_plain_step_and_float64(decoupled, warmup):
    from movenet_amd.optim import ema_decay_at
    n, band, steps = 1027, 256, 12           # 1027: no multiple of 4, two blocks of 256 threads x 4 elements
    ranges = [(5, 11), (1022, 1026)]         # begin and end inside a thread's four; the second in the last block
    skipped = np.zeros(n, dtype=bool)
    for lo, hi in ranges:
        skipped[lo:hi] = True
    gen = torch.Generator().manual_seed(11)
    SENT, ESENT = -7.25, 123.5               # the guard band's and the skipped averages' sentinels

    def padded(values):
        t = torch.full((n + band,), SENT, dtype=torch.float32)
        t[:n] = values
        return t.to(DEV)

    p0 = torch.randn(n, generator=gen)
    p, m, v = padded(p0), padded(torch.zeros(n)), padded(torch.zeros(n))
    tp, tm, tv = p.clone(), m.clone(), v.clone()  # the twin, stepped by mvn_adamw_step
    e0 = p0.clone()
    e0[torch.from_numpy(skipped)] = ESENT
    e = padded(e0)
    ref = e0.double().numpy().copy()
    big = float(max(p0.abs().max(), 0.0))
    worst = 0.0
    for t in range(steps):
        g = torch.randn(n, generator=gen).to(DEV)
        w = float(np.float32(1.0 - ema_decay_at(DECAY, t, warmup)))  # the float the kernel multiplies by
        _plain_step(tp, g, tm, tv, n, t + 1, decoupled, ranges)
        _ema_step(p, g, m, v, e, n, t + 1, decoupled, w, ranges)
        assert torch.equal(p, tp) and torch.equal(m, tm) and torch.equal(v, tv), t  # bits, the band included
        pn = p[:n].cpu().double().numpy()
        ref[~skipped] = ref[~skipped] + (pn[~skipped] - ref[~skipped]) * w
        en = e[:n].cpu().double().numpy()
        big = max(big, float(np.abs(pn).max()), float(np.abs(en[~skipped]).max()))
        worst = max(worst, float(np.abs(en - ref)[~skipped].max()))
    assert not torch.equal(tp[:n].cpu(), p0)                       # (it stepped)
    assert torch.equal(tp[:n].cpu()[torch.from_numpy(skipped)], p0[torch.from_numpy(skipped)])
    en = e.cpu()
    print(f"ema: worst |error| {worst:.3e}, bound {_ema_bound(big):.3e} (M = {big:.3f})")
    assert worst <= _ema_bound(big)
    assert (en[:n][torch.from_numpy(skipped)] == ESENT).all()      # skipped: bit-unchanged
    assert not (en[:n][torch.from_numpy(~skipped)] == ESENT).any()
    for buf in (e, p, m, v):                                       # nothing behind element n
        assert (buf[n:].cpu() == SENT).all()


def test_kernel_edge_sizes():
    p = torch.tensor([1.5, -7.25], device=DEV)
    g, m, v = torch.tensor([0.5, 9.0], device=DEV), torch.zeros(2, device=DEV), torch.zeros(2, device=DEV)
    e = torch.tensor([1.5, -7.25], device=DEV)
    tp, tm, tv = p.clone(), m.clone(), v.clone()
    _plain_step(tp, g, tm, tv, 1, 1, 1, [])
    _ema_step(p, g, m, v, e, 1, 1, 1, 0.25, [])
    assert torch.equal(p, tp) and torch.equal(m, tm) and torch.equal(v, tv)
    assert p[0].item() != 1.5 and p[1].item() == -7.25 and e[1].item() == -7.25
    want = np.float32(1.5) + (np.float32(p[0].item()) - np.float32(1.5)) * np.float32(0.25)
    assert abs(e[0].item() - float(want)) <= 2.0 ** -22
    before = [t.clone() for t in (p, m, v, e)]
    _ema_step(p, g, m, v, e, 0, 1, 1, 0.25, [])  # n == 0: MVN_OK, nothing written
    assert all(torch.equal(a, b) for a, b in zip(before, (p, m, v, e)))


# ---- 2. FlatAdamW with the average, against torch ---------------------------------------------------------------
@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "adam"])
def test_flat_adamw_ema_matches_torch(decoupled):
    from movenet_amd.optim import FlatAdamW, ema_decay_at
    torch.manual_seed(5)
    shapes = [(7, 5), (33,), (3, 11, 3), (129,)]  # 1: never a gradient; 3: gradients in a storage of their own
    ref = [torch.nn.Parameter(torch.randn(s, device=DEV)) for s in shapes]
    init = [p.detach().clone() for p in ref]
    kw = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    topt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(ref, **kw)
    mine = [torch.nn.Parameter(t.clone()) for t in init]
    off_ = [torch.nn.Parameter(t.clone()) for t in init]
    fopt = FlatAdamW(mine, decoupled=decoupled, ema_decay=DECAY, ema_warmup=True, **kw)
    plain = FlatAdamW(off_, decoupled=decoupled, **kw)  # ema_decay = 0: the launches to compare with
    assert not hasattr(plain, "ema") and fopt.ema.data_ptr() != fopt.flat.data_ptr()
    avg = [t.double().cpu() for t in init]
    sizes = [p.numel() for p in ref]
    big = max(float(t.abs().max()) for t in init)
    for step in range(8):
        flat = torch.randn(sum(sizes), device=DEV)
        off = 0
        for i, k in enumerate(sizes):
            g = flat[off:off + k].view(shapes[i])
            off += k
            for ps, own in ((ref, True), (mine, False), (off_, False)):
                ps[i].grad = None if i == 1 else (g.clone() if own or i == 3 else g)
        topt.step()
        fopt.step()
        plain.step()
        assert fopt.last_launches == plain.last_launches == 2  # the flat span (1 is a skip range) + parameter 3
        w = float(np.float32(1.0 - ema_decay_at(DECAY, step, True)))
        for i, (pr, pm) in enumerate(zip(ref, mine)):
            assert rel_err(pm.detach().cpu(), pr.detach().cpu()) < 1e-6, (step, i)  # as test_flat_adamw_matches_torch
            if i != 1:
                avg[i] = avg[i] + (pr.detach().double().cpu() - avg[i]) * w
            big = max(big, float(pr.detach().abs().max()))
    assert fopt.ema_updates == 8
    with fopt.averaged_parameters():
        got = [p.detach().clone() for p in mine]
    for i, (pr, pm, po) in enumerate(zip(ref, mine, off_)):
        assert torch.equal(pm.detach(), po.detach()), i                 # and the average costs the step no bit
        tol = _ema_bound(big) + 1e-6 * float(pr.detach().abs().max())
        err = float((got[i].double().cpu() - avg[i]).abs().max())
        assert err <= tol, (i, err, tol)
    assert torch.equal(got[1], init[1]) and torch.equal(mine[1].detach(), init[1])  # never moved: its own average
    assert not torch.equal(got[0], mine[0].detach())


def test_flat_adamw_ema_arguments():
    from movenet_amd.optim import FlatAdamW
    for bad in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            FlatAdamW([torch.nn.Parameter(torch.zeros(3, device=DEV))], ema_decay=bad)
    opt = FlatAdamW([torch.nn.Parameter(torch.zeros(3, device=DEV))])
    assert opt.ema_decay == 0.0 and not hasattr(opt, "ema") and "ema" not in opt.state_dict()["state"]["flat"]


# ---- 3. the zero-copy swap ---------------------------------------------------------------------------------------
SWAP = dict(layer_size=3, stack_size=2, input_channels=64, residual_channels=64, skip_channels=64)


def _inside(t: torch.Tensor, buf: torch.Tensor) -> bool:
    return buf.data_ptr() <= t.data_ptr() and t.data_ptr() + 4 * t.numel() <= buf.data_ptr() + 4 * buf.numel()


def test_averaged_parameters_swap_views_without_a_copy():
    from movenet_amd.ops import wavenet_forward_loss
    from movenet_amd.optim import FlatAdamW, order_like_backward
    from movenet_amd.wavenet import WaveNet
    model = WaveNet(**SWAP)
    model.load_state_dict(make_state_dict(**SWAP, seed=2))
    model.to(DEV).train()
    opt = FlatAdamW(order_like_backward(model), lr=3e-3, ema_decay=DECAY)
    x = one_hot(synthetic_indices(2, 100, 64, 9), 64).to(DEV)
    for _ in range(3):
        loss, _, _ = wavenet_forward_loss(model, x)
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
    model.eval()
    optimized = list(opt._params)
    with torch.no_grad():
        raw_out = model(x)
    raw = [p.detach().clone() for p in optimized]
    fresh = WaveNet(**SWAP)
    fresh.load_state_dict(opt.ema_state_dict(model))
    fresh.to(DEV).eval()

    def check_back():
        assert all(_inside(p, opt.flat) for p in optimized)
        assert all(torch.equal(p.detach(), r) for p, r in zip(optimized, raw))

    with opt.averaged_parameters():
        assert all(_inside(p, opt.ema) for p in optimized)
        with torch.no_grad():
            avg_out = model(x)
            assert torch.equal(avg_out, fresh(x))
        assert not torch.equal(avg_out, raw_out)
        with pytest.raises(RuntimeError, match="averaged_parameters"):
            with opt.averaged_parameters():
                pass
        assert all(_inside(p, opt.ema) for p in optimized)  # (the refused inner one left the outer one alone)
        with pytest.raises(RuntimeError, match="averaged_parameters"):
            opt.step()
    check_back()
    with pytest.raises(KeyError):
        with opt.averaged_parameters():
            raise KeyError("inside")
    check_back()
    with torch.no_grad():
        assert torch.equal(model(x), raw_out)
    with opt.averaged_parameters():  # usable again
        pass
    check_back()
    off = FlatAdamW([torch.nn.Parameter(torch.zeros(3, device=DEV))])
    with pytest.raises(RuntimeError, match="average is off"):
        with off.averaged_parameters():
            pass
    with pytest.raises(RuntimeError, match="average is off"):
        off.ema_state_dict(model)


# ---- 4. state round trip ------------------------------------------------------------------------------------------
def test_state_dict_round_trip_carries_the_average():
    from movenet_amd.optim import FlatAdamW
    torch.manual_seed(1)
    shapes = [(7, 5), (5,), (3, 4, 2), (11,)]
    init = [torch.randn(s, device=DEV) for s in shapes]
    grads = [[torch.randn(s, device=DEV) for s in shapes] for _ in range(4)]

    def run(opt, ps, steps):
        for g in steps:
            for p, gi in zip(ps, g):
                p.grad = gi.clone()
            opt.step()

    a_p = [torch.nn.Parameter(t.clone()) for t in init]
    a = FlatAdamW(a_p, lr=3e-3, weight_decay=0.05, ema_decay=DECAY)
    run(a, a_p, grads[:3])
    saved = copy.deepcopy(a.state_dict())
    assert saved["state"]["flat"]["ema_updates"] == 3 and torch.equal(saved["state"]["flat"]["ema"], a.ema)
    b_p = [torch.nn.Parameter(p.detach().clone()) for p in a_p]
    b = FlatAdamW(b_p, lr=1.0, weight_decay=0.0, ema_decay=DECAY)
    assert torch.equal(b.ema, b.flat)  # (a new average starts at the parameters)
    b.load_state_dict(saved)
    assert torch.equal(b.ema, a.ema) and b.ema_updates == a.ema_updates == 3 and b.state["flat"]["ema"] is b.ema
    run(a, a_p, grads[3:])
    run(b, b_p, grads[3:])
    assert torch.equal(b.ema, a.ema) and torch.equal(b.flat, a.flat) and b.ema_updates == 4
    # a state saved with the average off, loaded into an optimizer that has it on
    c_p = [torch.nn.Parameter(t.clone()) for t in init]
    c = FlatAdamW(c_p, lr=3e-3, weight_decay=0.05)
    run(c, c_p, grads[:3])
    saved = copy.deepcopy(c.state_dict())
    assert "ema" not in saved["state"]["flat"] and "ema_updates" not in saved["state"]["flat"]
    d_p = [torch.nn.Parameter(p.detach().clone()) for p in c_p]
    d = FlatAdamW(d_p, lr=3e-3, weight_decay=0.05, ema_decay=DECAY)
    run(d, d_p, grads[:1])  # (its average and count move away first)
    with torch.no_grad():
        d.flat.copy_(c.flat)
    d.load_state_dict(saved)
    assert torch.equal(d.ema, d.flat) and torch.equal(d.ema, c.flat) and d.ema_updates == 0
    assert torch.equal(d.exp_avg, c.exp_avg)


# ---- 5. the trainer -----------------------------------------------------------------------------------------------
SPEC = "synthetic://clips=6,frames=600,seed=5"


def _fit(tmp_path, name, precision=32, callbacks=None, **over):
    from movenet_amd.config import ModelConfig, TrainingConfig
    from movenet_amd.pytorch_lightning_trainer import Dance2Music, Trainer
    mc = ModelConfig(layer_size=4, stack_size=2, input_channels=64, residual_channels=64, skip_channels=64)
    kw = dict(model_config=mc, batch_size=2, val_batch_size=2, n_epochs=2, use_video=False, optimizer="AdamW",
              learning_rate=3e-3, weight_decay=0.01, model_output_path=tmp_path / name, gradient_clipping=0.0)
    cfg = TrainingConfig(**{**kw, **over})
    m = Dance2Music(SPEC, cfg)
    m.model.load_state_dict(make_state_dict(4, 2, 64, 64, 64, seed=5))
    tr = Trainer(max_epochs=cfg.n_epochs, default_root_dir=tmp_path / name, precision=precision,
                 callbacks=callbacks)
    return m, tr, mc


def _last_checkpoint(tmp_path, name):
    return torch.load(tmp_path / name / "checkpoints" / "epoch=1-step=6.ckpt", map_location="cpu", weights_only=True)


def _val_loss(m, mc, path, ema: bool) -> float:
    """Batch-size-weighted loss of a fresh model, loaded from the checkpoint's raw or averaged weights, over the
    module's validation batches (under the module's loss rule)."""
    from movenet_amd.checkpoint import load_into
    from movenet_amd.wavenet import WaveNet
    fresh = WaveNet(**asdict(mc))
    load_into(fresh, path, ema=ema)
    fresh.loss_rule = m.model.loss_rule
    fresh.to(DEV).eval()
    total, count = 0.0, 0
    with torch.no_grad():
        for batch in m.val_dataloader():
            loss, _, _ = fresh(batch.audio.to(DEV), None, return_loss=True)
            total += float(loss.double()) * batch.audio.shape[0]
            count += batch.audio.shape[0]
    assert count == 6
    return total / count


def _record_forward_pointers(m):
    """{"train": [...], "validation": [...]}: where the model's first parameter points at every forward of the
    module's training_step / validation_step (a pre-hook on the WaveNet; the step tells which list)."""
    forwards, phase = {"train": [], "validation": []}, []
    m.model.register_forward_pre_hook(
        lambda mod, args: forwards[phase[-1]].append(next(mod.parameters()).data_ptr()) if phase else None)
    for name, key in (("training_step", "train"), ("validation_step", "validation")):
        def step(*a, _inner=getattr(m, name), _key=key, **k):
            phase.append(_key)
            try:
                return _inner(*a, **k)
            finally:
                phase.pop()
        setattr(m, name, step)
    return forwards


def test_trainer_validates_samples_and_saves_the_average(tmp_path):
    from movenet_amd.callbacks import LogSamplesCallback
    from movenet_amd.optim import FlatAdamW
    seen = {"train": [], "validation": []}
    fresh_ptrs = []

    class Recording(LogSamplesCallback):
        def log_samples(self, split, *a, **k):
            seen[split].extend(fresh_ptrs)
            del fresh_ptrs[:]
            return super().log_samples(split, *a, **k)

    m, tr, mc = _fit(tmp_path, "ema", callbacks=[Recording(log_every_n_epochs=1)], ema_decay=DECAY,
                     log_samples_every=1, generate_n_samples=40)
    generate = m.model.generate

    def recording_generate(*a, **k):
        fresh_ptrs.append(next(m.model.parameters()).data_ptr())
        return generate(*a, **k)

    m.model.generate = recording_generate
    forwards = _record_forward_pointers(m)
    tr.fit(m)
    opt = tr.optimizer
    assert isinstance(opt, FlatAdamW) and opt is m.ema_optimizer and opt.ema_updates == 6
    lo, hi = opt.ema.data_ptr(), opt.ema.data_ptr() + 4 * opt.ema.numel()
    assert len(seen["train"]) == 6 and len(seen["validation"]) == 6 and not fresh_ptrs  # 2 epochs x 3 batches each
    assert all(lo <= q < hi for q in seen["train"] + seen["validation"])
    # the forward of every validation_step read the averaged weights, that of every training_step the raw ones
    flo, fhi = opt.flat.data_ptr(), opt.flat.data_ptr() + 4 * opt.flat.numel()
    assert len(forwards["train"]) == 6 and len(forwards["validation"]) == 6
    assert all(lo <= q < hi for q in forwards["validation"]) and all(flo <= q < fhi for q in forwards["train"])
    assert all(_inside(p, opt.flat) for p in m.model.parameters())  # after fit: the raw iterate again
    assert (tmp_path / "ema" / "samples" / "train" / "epoch=1-batch=2-clip=0-gen.wav").exists()
    assert (tmp_path / "ema" / "samples" / "validation" / "epoch=1-batch=2-clip=0-gen.wav").exists()
    ck = _last_checkpoint(tmp_path, "ema")
    assert ck["ema_decay"] == DECAY and ck["ema_updates"] == 6
    want = opt.ema_state_dict(m.model)
    assert sorted(ck["ema_state_dict"]) == sorted(ck["state_dict"]) == sorted(f"model.{k}" for k in want)
    assert all(torch.equal(ck["ema_state_dict"][f"model.{k}"], v.cpu()) for k, v in want.items())
    # every tensor that training moved has an average that lags it (the rest -- the unused video and context
    # parameters, the last layer's residual conv -- equal their averages)
    sd0 = make_state_dict(4, 2, 64, 64, 64, seed=5)
    stepped = [k for k in want if not torch.equal(ck["state_dict"][f"model.{k}"], sd0[k])]
    assert len(stepped) > 10
    for k in want:
        same = torch.equal(ck["state_dict"][f"model.{k}"], ck["ema_state_dict"][f"model.{k}"])
        assert same == (k not in stepped), k
    assert all(torch.equal(ck["state_dict"][f"model.{k}"], v.cpu()) for k, v in m.model.state_dict().items())
    # val_loss is the averaged weights': a fresh model, loaded from the file, over the same validation batches
    # (on this noise the reference rule's loss sits at ln Q for either set of weights, so this figure alone does not
    # tell them apart: the forward pointers above and the model-rule run below do)
    path = tmp_path / "ema" / "checkpoints" / "epoch=1-step=6.ckpt"
    assert abs(tr.val_epoch_means["val_loss"] - _val_loss(m, mc, path, ema=True)) <= 1e-6
    # the train metrics are the raw iterate's: the same run without the average logs the same train losses
    m0, tr0, _ = _fit(tmp_path, "off")
    tr0.fit(m0)
    assert [h["train_loss"] for h in tr0.history] == [h["train_loss"] for h in tr.history]
    ck0 = _last_checkpoint(tmp_path, "off")
    assert not {"ema_state_dict", "ema_decay", "ema_updates"} & set(ck0)
    assert isinstance(tr0.optimizer, FlatAdamW) and not hasattr(tr0.optimizer, "ema") and m0.ema_optimizer is None
    assert all(torch.equal(ck0["state_dict"][k], ck["state_dict"][k]) for k in ck["state_dict"])


def test_trainer_val_loss_is_the_averaged_weights_not_the_raw_ones(tmp_path):
    """The same model and clips in a setting that keeps the two sets of weights far apart, under the model loss rule,
    whose loss is not confined to ln Q: a constant learning rate of 1e-2 (no scheduler) moves every raw weight by up to
    6e-2 in the six steps, and without warm-up the average still holds 0.9^6 = 53 % of the initial weights after them.
    The reported val_loss is that of the checkpoint's averaged weights to 1e-6, and the raw weights' loss lies clearly
    outside that tolerance (ten times it), so a validation loop on the raw iterate would fail the first assertion.
    (Under the issue's own setting -- one-cycle schedule ending at lr 1.2e-8, warm-up on, noise clips -- the two losses
    are 2.7e-6 apart, 4.1634251 against 4.1634278: outside 1e-6, but not clearly.)"""
    m, tr, mc = _fit(tmp_path, "model_rule", ema_decay=DECAY, ema_warmup=False, loss_rule="model", scheduler=None,
                     learning_rate=1e-2)
    tr.fit(m)
    path = tmp_path / "model_rule" / "checkpoints" / "epoch=1-step=6.ckpt"
    averaged, raw = _val_loss(m, mc, path, ema=True), _val_loss(m, mc, path, ema=False)
    got = tr.val_epoch_means["val_loss"]
    print(f"val_loss {got:.7f}, averaged weights {averaged:.7f}, raw weights {raw:.7f}")
    assert abs(got - averaged) <= 1e-6
    assert abs(got - raw) > 1e-5
    assert abs(tr.val_epoch_means["val_bits_per_sample"] - averaged / np.log(2.0)) <= 2e-6


def test_trainer_bf16_with_the_average(tmp_path):
    m, tr, _ = _fit(tmp_path, "bf16", precision="bf16", ema_decay=DECAY)
    tr.fit(m)
    ck = _last_checkpoint(tmp_path, "bf16")
    assert ck["ema_updates"] == 6 and all(torch.isfinite(v).all() for v in ck["ema_state_dict"].values())
    assert np.isfinite(tr.val_epoch_means["val_loss"]) and torch.isfinite(tr.optimizer.ema).all()
    assert all(_inside(p, tr.optimizer.flat) for p in m.model.parameters())


def test_trainer_refuses_the_average_without_the_fused_step(tmp_path):
    from movenet_amd.config import arg_parser, config_from_args
    from movenet_amd.pytorch_lightning_trainer import Dance2Music
    args = arg_parser().parse_args(["--dataset", SPEC, "--ema_decay", "0.9", "--optimizer", "SGD", "--use_video", "0",
                                    "--input_channels", "64", "--layer_size", "2", "--stack_size", "2"])
    m = Dance2Music(SPEC, config_from_args(args)).to(DEV)
    with pytest.raises(ValueError, match="--ema_decay"):
        m.configure_optimizers()
