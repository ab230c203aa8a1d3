"""GPU: the layer kernels compute what they computed BEFORE their bodies were shared -- the two one-kernel layer
backward kernels (csrc/bwd_layer64_body.inc), the forward strip kernels (csrc/fwd_layer64s_body.inc) and the two
256-thread passes of the two-half backward (csrc/bwd_half64_body.inc): SHA-256 of the logits, of every parameter
gradient and of the context's gradient, for one training step per mode, against a recording made on an MI355X from a
library built at the commit before such a change (tests/golden/layer_kernels_sha256.json; its header names the commit,
the device and its CU count).  The fixture also holds the hashes of every case's input bytes, so that an input that
drifted is told apart from a kernel that changed.

One case per mode, each asserting its ``mvn_last_backward_form()``:

    fp32          MVN_BWD_FORM_ONE          bwd_layer64_kernel<false>
    fp32-ctx      MVN_BWD_FORM_ONE          bwd_layer64_kernel<true> (df | dg written for the context pass)
    fp32-label    MVN_BWD_FORM_ONE_GLOBAL   bwd_layer64_kernel<true> and the row-sum kernel
    bf16          MVN_BWD_FORM_BF16         bwd_layer64_bf16_kernel<false, false>
    bf16-label    MVN_BWD_FORM_BF16_GLOBAL  bwd_layer64_bf16_kernel<true, false> (row sums inside the kernel)
    bf16-ctx      MVN_BWD_FORM_BF16_CTX     bwd_layer64_bf16_kernel<false, true>
    fp32-mfma     MVN_BWD_FORM_ONE          as fp32, behind fused_layer64s_kernel<false>
    fp32-mfma-ctx MVN_BWD_FORM_ONE          as fp32-ctx, behind fused_layer64s_kernel<true>
    fp32-halves   MVN_BWD_FORM_HALVES       bwd_dz_wgrs64_kernel and bwd_dx_wgfg64_kernel (MOVENET_HIP_BWD_FORM=split)
    fp32-ctx-halves MVN_BWD_FORM_HALVES     both halves and bwd_dctx_wgctx64_kernel in the first half's chunks (split)

and the forward of each mode runs the matching strip kernel (fused_layer64s_bf3_kernel<false | true>,
fused_layer64s_ctxw2_kernel, fused_layer64s_bf16_kernel<...>), all of them one body (csrc/fwd_layer64s_body.inc).  The
two fp32-mfma cases run under MOVENET_HIP_FORWARD_MFMA=f32, which keeps the layers on the fp32-MFMA strip kernels
(fused_layer64s_kernel<false | true>) that no other case reaches.  What is hashed: the logits; the forward's saved
tensors, read from the pass's buffers before the backward runs -- tanh and sigmoid of every layer over its valid columns [t_lo, T) and the
skip sum over [RF - 1, T) --; the gradient of every parameter -- the layers' weights and biases, the head, the context
convs (the label's come from ``rowsum``), ``global_embedding.weight`` (from ``de``) -- and, in the context modes,
``dctx`` as the gradient of the context leaf.  The saved tensors tell a forward that changed from a backward that did.

Shape: C = K = 64, layer_size 3, stack_size 2 (dilations 1, 2, 4, 1, 2, 4; receptive field 16), Q = 64, batch 32,
T = 2600 = 40 x 64 + 40.  fp32-ctx and fp32-mfma-ctx run at Q = 128: the fp32 plan keeps the conditioned layers' second
A' | P0 pair in the dlogit tensor, which holds it from Q = 128 on; at Q = 64 it takes the two-half form and
bwd_layer64_kernel<true> does not run there (the layer kernels never see Q).  The two halves cases run at Q = 128 as
well: both halves' slabs of a layer lie in da1 at once, 14 x 32 x 8192 + 7 x 32 x 16384 = 7.34 M floats (and 57 344 bias
partials), which da1 holds at Q = 128 and not at Q = 64; with less the plan takes the two-kernel forms.

* Tiles.  A layer's t_lo is 1, 3, 7, 8, 10 or 14, never a multiple of 64: tile 0 is an edge tile, so is tile 40 (columns
  2560 .. 2599), and tiles 1 .. 39 are interior (tile 39 ends at 2560, and 2560 + up_d <= 2600).
* Backward chunks (fb_chunks_on, then bwd_layer64_plan's recut where the slab scratch is smaller).  On 256 CUs a
  sequence gets at most 256 / 32 = 8 chunks: 41 tiles in chunks of 6, that is 7 chunks, the last one tiles 36 .. 40.  A
  scratch that holds n < 7 workgroups per sequence recuts to ceil(41 / n) tiles per chunk, and for every n the last chunk
  keeps at least five tiles (n = 6: 6 x 7, last 6; 5: 9, last 5; 4: 11, last 8; 3: 14, last 13; 2: 21, last 20).  So in
  every case, whichever cut its scratch gives, a workgroup walks at least five tiles: its first tile loaded in front of
  the loop (edge in chunk 0, interior elsewhere), interior tiles prefetched in parts between the slots (spread), and in
  the last chunk the edge tile 40 prefetched inside the loop (gload_r_edge, set_zero_flags(.., false)).
  test_chunk_arithmetic checks this paragraph with the planner's formula.
* The halves' chunks (bwd_pass256_fits, bwd_dx_wgfg64_fits).  The first half and the context pass run two workgroups per
  CU: 16 chunks wanted, 41 tiles in chunks of 3, that is 14 chunks, the last one tiles 39 .. 40.  Every workgroup
  prefetches at least one tile inside its loop; chunk 0 loads the edge tile 0 in front of the loop, the last chunk
  prefetches the edge tile 40 inside it.  In fp32-ctx-halves the context pass runs in exactly these chunks from the
  same scratch (fp32-ctx has it in the layer kernel's chunks of 6).  The second half runs one workgroup per CU: the
  7 chunks of 6 above, interior tiles prefetched in parts, tile 40 prefetched by gload_edge inside the loop.
* Forward chunks (fb_chunks with a granule of 8 waves x 32 columns = 256): ceil(2600 / 256) = 11 rounds over at most 8
  chunks, so a chunk is 2 rounds = 512 columns: every wave of chunks 0 .. 4 takes two strips (next-strip prefetch with a
  live next strip, the old-skip loads across strips), the last chunk holds columns 2560 .. 2599 only.

Chunking, and with it the summation order of the weight gradients, depends on the CU count: on a device with another
count than the recording's the test skips with that reason.

Inputs are integer arithmetic in numpy (an index hash): no RNG stream, no transcendental.  Weights come from
make_state_dict.

Before the recording the parent's library ran every case twice, in separate processes: every tensor of every case
came out with the same bytes both times, so none is left out of the fixture.  (The fixture was recorded again, all
eight cases from one library, when the two fp32-mfma cases joined: the two new cases reproduced in two processes, and
the six older cases' hashes came out as in the first recording.  Likewise when the two halves cases joined: each ran
twice in separate processes from the parent's library, every tensor came out with the same bytes both times, so none is
left out; the eight older cases' hashes are the ones recorded before.)

Recording: with MOVENET_LAYER_KERNELS_RECORD=<commit> the test writes the fixture instead of comparing.  That is only
worth something from the parent's library, so it refuses to run unless MOVENET_HIP_LIB names the library to record
from (built at <commit>):

    MOVENET_HIP_LIB=<library built at that commit> MOVENET_LAYER_KERNELS_RECORD=<commit> \\
        python -m pytest tests/test_layer_kernel_bits_gpu.py
"""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from movenet_amd import _native as N
from movenet_amd import ops
from movenet_amd.utils.weights import make_state_dict

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layer_kernels_sha256.json")
RECORD = os.environ.get("MOVENET_LAYER_KERNELS_RECORD")
DEV = "cuda:0"
B, T, C, G, RF, CUS = 32, 2600, 64, 4, 16, 256
T_LO = (1, 3, 7, 8, 10, 14)  # first valid column of each layer's outputs: the dilations summed
CTX = "context"  # the key the gradient of the context is filed under

# case -> (forward_precision, conditioning, Q, expected backward form, the case's environment)
MFMA_F32, SPLIT = {"MOVENET_HIP_FORWARD_MFMA": "f32"}, {"MOVENET_HIP_BWD_FORM": "split"}
CASES = {
    "fp32": ("fp32", None, 64, N.BWD_FORM_ONE, {}),
    "fp32-ctx": ("fp32", "ctx", 128, N.BWD_FORM_ONE, {}),
    "fp32-label": ("fp32", "label", 64, N.BWD_FORM_ONE_GLOBAL, {}),
    "bf16": ("bf16", None, 64, N.BWD_FORM_BF16, {}),
    "bf16-label": ("bf16", "label", 64, N.BWD_FORM_BF16_GLOBAL, {}),
    "bf16-ctx": ("bf16", "ctx", 64, N.BWD_FORM_BF16_CTX, {}),
    "fp32-mfma": ("fp32", None, 64, N.BWD_FORM_ONE, MFMA_F32),
    "fp32-mfma-ctx": ("fp32", "ctx", 128, N.BWD_FORM_ONE, MFMA_F32),
    "fp32-halves": ("fp32", None, 128, N.BWD_FORM_HALVES, SPLIT),
    "fp32-ctx-halves": ("fp32", "ctx", 128, N.BWD_FORM_HALVES, SPLIT),
}


def _cfg(Q):
    return dict(layer_size=3, stack_size=2, input_channels=Q, residual_channels=C, skip_channels=C)


def _hash(n: np.ndarray, seed: int) -> np.ndarray:
    """int64 -> [0, 2^31): two rounds of a linear congruence with a shift between them"""
    v = ((n + 7919 * seed) * 1103515245 + 12345) % (1 << 31)
    return ((v ^ (v >> 13)) * 1664525 + 1013904223) % (1 << 31)


def _values(shape, seed: int, bits: int) -> torch.Tensor:
    """fp32 multiples of 2^-bits in [-1, 1)"""
    n = np.arange(int(np.prod(shape)), dtype=np.int64)
    v = (_hash(n, seed) >> 9) % (1 << (bits + 1)) - (1 << bits)
    return torch.from_numpy((v.astype(np.float32) / np.float32(1 << bits)).reshape(shape))


@functools.lru_cache(maxsize=None)
def _inputs(Q):
    idx = torch.from_numpy(((_hash(np.arange(B * T, dtype=np.int64), 1) >> 11) % Q).reshape(B, T))
    x = torch.zeros(B, Q, T).scatter_(1, idx[:, None, :], 1.0)
    return dict(x=x, up=_values((B, Q, T - RF), 2, 10), ctx=_values((B, C, T), 3, 8), E=_values((G, C), 4, 6),
                labels=torch.from_numpy((_hash(np.arange(B, dtype=np.int64), 5) >> 7) % G))


@functools.lru_cache(maxsize=None)
def _weights(Q):
    return make_state_dict(**_cfg(Q), seed=7)


def _sha(t: torch.Tensor) -> str:
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def _forward_buffers(out: torch.Tensor):
    """the ForwardBuffers of the pass that produced ``out`` (kept by its autograd node for the backward)"""
    todo, seen = [out.grad_fn], set()
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if getattr(getattr(fn, "buf", None), "th", None) is not None:
            return fn.buf
        todo.extend(f for f, _ in fn.next_functions)
    raise AssertionError("no node of the graph holds the forward's buffers")


def _chunks(nt: int, per_seq: int, tile: int) -> tuple:
    """fb_chunks_on (csrc/fused_bwd.h) for ``per_seq`` wanted chunks: (chunks, tiles per chunk, tiles of the last chunk)"""
    tiles = -(-nt // tile)
    per_chunk = max(1, -(-tiles // per_seq))
    chunks = -(-tiles // per_chunk)
    return chunks, per_chunk, tiles - (chunks - 1) * per_chunk


def test_chunk_arithmetic():
    """The docstring's claims about the shape, with the planner's formula (no kernel runs, no GPU needed)."""
    assert all(t % 64 for t in T_LO) and T % 64 and max(T_LO) == RF - 2
    assert 39 * 64 + 64 + 4 <= T  # tile 39 is interior for every up_d <= 4
    assert _chunks(T, CUS // B, 64) == (7, 6, 5)
    for n in range(1, CUS // B + 1):  # whatever the slab scratch holds: the last chunk has an interior and the edge tile
        chunks, per_chunk, last = _chunks(T, n, 64)
        assert chunks <= n and last >= 5 and per_chunk >= 5, (n, chunks, per_chunk, last)
    assert _chunks(T, CUS // B, 256) == (6, 2, 1)  # forward: two strips per wave in chunks 0 .. 4
    # the halves (MOVENET_HIP_BWD_FORM=split).  A layer's tiles start at (t_lo & ~31) = 0: its span is T for every layer
    assert all(t < 32 for t in T_LO)
    # first half and context pass, two workgroups per CU: every workgroup prefetches inside its loop (>= 2 tiles), chunk 0
    # starts on the edge tile 0, the last chunk is tiles 39 .. 40 and prefetches the edge tile 40
    assert _chunks(T, 2 * CUS // B, 64) == (14, 3, 2) and 13 * 3 == 39 and 40 * 64 < T < 41 * 64
    # second half, one per CU: interior tiles prefetched in parts, the last chunk tiles 36 .. 40 with the edge tile
    # prefetched in the loop
    assert _chunks(T, CUS // B, 64) == (7, 6, 5)
    # both halves' slabs of a layer and the first half's bias partials: in da1 (B, Q, Sp >= T - RF) at Q = 128, not at 64
    need = 14 * B * 128 * 64 + 7 * B * 128 * 128 + 14 * B * 128
    assert B * 64 * T < need <= B * 128 * (T - RF)


def run_case(case: str) -> dict:
    """One training step of ``case`` (the caller has set the case's environment)."""
    from movenet_amd.wavenet import WaveNet
    precision, cond, Q, form, _ = CASES[case]
    inp, full = _inputs(Q), _weights(Q)
    if cond == "label":
        m = WaveNet(**_cfg(Q), global_classes=G)
        m.load_state_dict({**full, "global_embedding.weight": inp["E"]}, strict=True)
        m.global_path = "bias"
    else:
        m = WaveNet(**_cfg(Q))
        m.load_state_dict(dict(full), strict=False)
    m.forward_precision = precision
    m.bf16_context = cond == "ctx"
    m = m.to(DEV).train()
    x, ctx = inp["x"].to(DEV), None
    if cond == "label":
        out = m(x, None, inp["labels"].to(DEV), output_unnormalized=False)
    else:
        ctx = inp["ctx"].to(DEV).requires_grad_(True) if cond == "ctx" else None
        out = ops.wavenet_forward(m, x, ctx, output_unnormalized=False)
    assert tuple(out.shape) == (B, Q, T - RF), tuple(out.shape)
    got = {"input." + k: _sha(v) for k, v in inp.items()}
    got["logits"] = _sha(out)
    buf = _forward_buffers(out)  # (read before the backward, which may reuse the pass's scratch)
    assert tuple(buf.th.shape[:3]) == (len(T_LO), B, C) and tuple(buf.skip.shape[:2]) == (B, C)
    for l, t_lo in enumerate(T_LO):
        got[f"saved.tanh.{l}"] = _sha(buf.th[l, :, :, t_lo:T])
        got[f"saved.sigmoid.{l}"] = _sha(buf.sg[l, :, :, t_lo:T])
    got["saved.skip"] = _sha(buf.skip[:, :, RF - 1:T])  # (column = time: t_base = (RF - 1) & ~31 = 0)
    (out * inp["up"].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert N.lib().mvn_last_backward_form() == form, (case, N.lib().mvn_last_backward_form())
    grads = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads.values())
    got.update({"grad." + k: _sha(g) for k, g in grads.items()})
    if ctx is not None:
        got["grad." + CTX] = _sha(ctx.grad)
    return got


def _record(case: str, got: dict) -> None:
    assert os.environ.get("MOVENET_HIP_LIB"), __doc__
    props = torch.cuda.get_device_properties(0)
    head = {"recorded_from_commit": RECORD, "device": props.name, "compute_units": props.multi_processor_count}
    out = {}
    if os.path.exists(FIXTURE):
        with open(FIXTURE) as f:
            out = json.load(f)
    if {k: out.get(k) for k in head} != head:
        out = dict(head, what="SHA-256 of the input bytes, the logits, the saved tensors and every gradient of "
                              "tests/test_layer_kernel_bits_gpu.py's cases, recorded on that device from a library built "
                              "at that commit", cases={})
    out["cases"][case] = got
    with open(FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_outputs_equal_the_recording(monkeypatch, case):
    for name, value in CASES[case][4].items():
        monkeypatch.setenv(name, value)  # (read again by the passes: MOVENET_DEBUG_GUARD)
    if not RECORD:
        with open(FIXTURE) as f:
            fixture = json.load(f)
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        if cus != fixture["compute_units"]:
            pytest.skip(f"recorded on {fixture['compute_units']} CUs, this device has {cus}: the layer pass cuts a "
                        "sequence into other chunks and sums the weight gradients in another order")
    got = run_case(case)
    if RECORD:
        _record(case, got)
        return
    want = fixture["cases"][case]
    print(f"{case}: " + ", ".join(f"{k} {'ok' if got[k] == want.get(k) else 'DIFFERS'}" for k in sorted(got)))
    assert {k: v for k, v in got.items() if k.startswith("input.")} == \
        {k: v for k, v in want.items() if k.startswith("input.")}, "the test's inputs drifted"
    assert got == want
