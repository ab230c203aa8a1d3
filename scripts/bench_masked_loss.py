"""What the per-sequence column counts cost: one MI355X, one process, the legs of each group interleaved
in rotating order, HIP events around each call, medians.

    python scripts/bench_masked_loss.py [--reps 30] [--out profiles/masked_loss.json]

* loss kernels on config 2's head tensor, (16, 256, 12928) fp32, both rules: mvn_softmax_ce_forward_ex / _backward_ex
  against the _len calls with every column counted and with every row half counted (the forward runs on a copy made
  outside the timed span);
* a config-2 train step (forward + loss + backward of the 30-layer model, 16 x 16000 samples): lengths=None twice, and
  full lengths;
* mvn_audio_frontend_var against mvn_audio_frontend on the same upload of 16 clips.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from movenet_amd import _native as N  # noqa: E402

DEV = "cuda:0"


def timed(legs: dict, reps: int, warmup: int = 3) -> dict:
    """legs: name -> (prepare or None, call).  Round r runs the legs rotated by r; returns per-leg statistics in us."""
    names = list(legs)
    times = {k: [] for k in names}
    for r in range(warmup + reps):
        for k in names[r % len(names):] + names[:r % len(names)]:
            prepare, call = legs[k]
            if prepare is not None:
                prepare()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            if r >= warmup:
                times[k].append(a.elapsed_time(b) * 1e3)
    return {k: dict(median_us=statistics.median(v), best_us=min(v), worst_us=max(v), reps=len(v))
            for k, v in times.items()}


def loss_kernels(reps: int) -> dict:
    lib, B, Q, S = N.lib(), 16, 256, 12928
    stream = torch.cuda.current_stream(DEV).cuda_stream
    g = torch.Generator().manual_seed(1)
    src = (torch.randn(B, Q, S, generator=g) * 4.0).to(DEV)
    tg = torch.randint(0, Q, (B, S), generator=g).to(DEV)
    x = torch.empty_like(src)
    parts = max(lib.mvn_ce_parts(B, S), 1)
    lp = torch.zeros(parts, dtype=torch.float32, device=DEV)
    cp = torch.zeros(parts, dtype=torch.int32, device=DEV)
    full = torch.full((B,), S, dtype=torch.int32, device=DEV)
    half = torch.full((B,), S // 2, dtype=torch.int32, device=DEV)
    Sp = lib.mvn_padded_len(S + 1)
    d = torch.empty(B, Q, Sp, dtype=torch.float32, device=DEV)
    out = {}
    for rule_name, rule in (("reference", N.LOSS_REFERENCE), ("model", N.LOSS_MODEL)):
        def prep():
            x.copy_(src)
            lp.zero_()
            cp.zero_()

        def fwd(valid):
            if valid is None:
                return lambda: N.check(lib.mvn_softmax_ce_forward_ex(x.data_ptr(), tg.data_ptr(), B, Q, S, lp.data_ptr(),
                                                                     cp.data_ptr(), rule, stream), "forward_ex")
            return lambda: N.check(lib.mvn_softmax_ce_forward_len(x.data_ptr(), tg.data_ptr(), B, Q, S, lp.data_ptr(),
                                                                  cp.data_ptr(), rule, valid.data_ptr(), stream),
                                   "forward_len")
        out[f"forward_{rule_name}"] = timed({"ex": (prep, fwd(None)), "len_full": (prep, fwd(full)),
                                             "len_half": (prep, fwd(half)), "ex_again": (prep, fwd(None))}, reps)
        prep()
        fwd(None)()  # x: probabilities, what the backward reads
        scale = 1.0 / (B * S)

        def bwd(valid):
            if valid is None:
                return lambda: N.check(lib.mvn_softmax_ce_backward_ex(x.data_ptr(), tg.data_ptr(), B, Q, S, scale, None,
                                                                      d.data_ptr(), Q * Sp, Sp, 0, S + 1, rule, stream),
                                       "backward_ex")
            return lambda: N.check(lib.mvn_softmax_ce_backward_len(x.data_ptr(), tg.data_ptr(), B, Q, S, scale, None,
                                                                   d.data_ptr(), Q * Sp, Sp, 0, S + 1, rule,
                                                                   valid.data_ptr(), stream), "backward_len")
        out[f"backward_{rule_name}"] = timed({"ex": (None, bwd(None)), "len_full": (None, bwd(full)),
                                              "len_half": (None, bwd(half)), "ex_again": (None, bwd(None))}, reps)
    return dict(shape=[B, Q, S], **out)


def train_step(reps: int) -> dict:
    from movenet_amd.utils.weights import make_state_dict, one_hot, synthetic_indices
    from movenet_amd.wavenet import WaveNet
    cfg = dict(layer_size=10, stack_size=3, input_channels=256, residual_channels=64, skip_channels=64)
    m = WaveNet(**cfg)
    m.load_state_dict(make_state_dict(**cfg, seed=1), strict=True)
    m = m.to(DEV).train()
    B, T = 16, 16000
    x = one_hot(synthetic_indices(B, T, 256, 3), 256).to(DEV)

    def step(lengths):
        def run():
            loss, _, _ = m(x, return_loss=True, lengths=lengths)
            loss.backward()
            m.zero_grad(set_to_none=True)
        return run
    res = timed({"none": (None, step(None)), "full_lengths": (None, step([T] * B)), "none_again": (None, step(None))},
                max(reps // 4, 5), warmup=2)
    return dict(batch=B, frames=T, **res)


def frontend(reps: int) -> dict:
    from movenet_amd.ops import audio_clip_descriptors, audio_clip_var_descriptors
    lib, B, N_OUT, Q = N.lib(), 16, 160000, 256
    stream = torch.cuda.current_stream(DEV).cuda_stream
    rng = np.random.default_rng(0)
    frames = [int(v) for v in rng.integers(100000, 441000, B)]
    channels = [1 + b % 2 for b in range(B)]
    pcm = torch.from_numpy(rng.integers(-20000, 20000, sum(f * c for f, c in zip(frames, channels)), dtype=np.int16)).to(DEV)
    plain = torch.from_numpy(audio_clip_descriptors(frames, channels)).to(DEV)
    n_out = [min(N_OUT, round(f * 16000 / 44100)) for f in frames]
    var = torch.from_numpy(audio_clip_var_descriptors(frames, channels, n_out)).to(DEV)
    y = torch.empty(B, N_OUT, dtype=torch.float32, device=DEV)
    idx = torch.empty(B, N_OUT, dtype=torch.int32, device=DEV)
    scratch = torch.empty(max(lib.mvn_audio_frontend_scratch_floats(B, N_OUT), 2), dtype=torch.float32, device=DEV)
    legs = {"plain": (None, lambda: N.check(lib.mvn_audio_frontend(pcm.data_ptr(), pcm.numel(), plain.data_ptr(), B, Q, N_OUT,
                                                                  1, y.data_ptr(), scratch.data_ptr(), idx.data_ptr(),
                                                                  stream), "frontend")),
            "var": (None, lambda: N.check(lib.mvn_audio_frontend_var(pcm.data_ptr(), pcm.numel(), var.data_ptr(), B, Q,
                                                                    N_OUT, 1, y.data_ptr(), scratch.data_ptr(),
                                                                    idx.data_ptr(), stream), "frontend_var"))}
    return dict(clips=B, width=N_OUT, n_out=n_out, **timed(legs, reps))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join("profiles", "masked_loss.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    result = dict(device=torch.cuda.get_device_name(0), reps=args.reps, loss_kernels=loss_kernels(args.reps),
                  train_step=train_step(args.reps), audio_frontend=frontend(args.reps))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
