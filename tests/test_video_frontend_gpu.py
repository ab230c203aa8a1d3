"""GPU: the video front end (mvn_video_frontend, ops.video_frontend) against the torch oracle
(tests/video_frontend_reference.py), and the WAV-folder loader's raw-frame path on the device.

Margins.  Output A of the oracle is the chain in fp32, output B the same with the interpolation in float64, d the
largest |A - B| before rounding on the very inputs of a case.

* Where every weight and partial sum is exact in fp32 (64 x 64: the identity; 256 x 128 without antialias: every weight
  0.5) the kernel must give A's bytes.
* General shapes: with delta = max(8 d, 1e-4), the level equals round_half_even(B) wherever B lies further than delta
  from a tie, |level - B| <= 0.5 + delta everywhere, and the pixels within delta of a tie are at most 1 % of the case
  (one launch of all seven clips under one setting).  Without antialias the output side being 64 makes every source
  position a multiple of 1 / 128, so torch's fp32 evaluation is exact (d = 0) and B's ties are exact ties -- the
  (64, 200) clip alone has 1 / 16 of its pixels on one (values are multiples of 1 / 16).  Measured with the seed
  below, on the CPU (the share depends on the oracle and the inputs alone): within delta of a tie are 849 of 86 016
  pixels, 0.99 % of the launch, without antialias (6.1 % of the (64, 200) clip, below 0.7 % of every other) and 187,
  0.22 %, with it; oracle A itself differs from round(B) at none without antialias and at 15 pixels, 0.017 %, with it.
  Where d is 0 the test also asks for A's bytes at every pixel, ties included, so no pixel of those clips goes unchecked.
"""
import numpy as np
import pytest
import torch

import video_frontend_reference as R
import wav_material as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD, FILL = 1001, 0xA5          # odd: `pix` and `levels` themselves start at odd addresses
SHAPES = ((100, 150), (37, 53), (48, 30), (1, 1), (64, 200), (65, 63), (333, 257))
N_FRAMES, SEED = 3, 20240


def _launch(frames, antialias, gaps=None, descriptors=None, **kw):
    """All clips (each (n, H, W[, 3]) uint8 numpy, the same n) in ONE launch, `pix` and `levels` carved out of
    guard-filled buffers, clip b at an offset moved by gaps[b] filler bytes.  Returns (levels, status, guards intact)."""
    from movenet_amd.ops import video_frontend
    n = frames[0].shape[0]
    shapes = [(f.shape[1], f.shape[2], 3 if f.ndim == 4 else 1) for f in frames]
    gaps = gaps or [0] * len(frames)
    offsets, at = [], 0
    for f, g in zip(frames, gaps):
        at += g
        offsets.append(at)
        at += f.size
    host = np.full(GUARD + at + GUARD, FILL, dtype=np.uint8)
    for f, o in zip(frames, offsets):
        host[GUARD + o:GUARD + o + f.size] = f.reshape(-1)
    raw = torch.from_numpy(host).to(DEV)
    pix = raw[GUARD:GUARD + at]
    size = len(frames) * n * 64 * 64
    raw_l = torch.full((GUARD + size + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    out = raw_l[GUARD:GUARD + size].view(len(frames), n, 64, 64)
    levels, status = video_frontend(pix, shapes, n, antialias=antialias, offsets=offsets, descriptors=descriptors,
                                    out=out, return_status=True, **kw)
    torch.cuda.synchronize()
    intact = (bool((raw_l[:GUARD] == FILL).all()) and bool((raw_l[GUARD + size:] == FILL).all())
              and torch.equal(raw.cpu(), torch.from_numpy(host)))
    return levels.cpu(), status.cpu(), intact


# ---- 1. gray, exhaustive -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def all_triples():
    v = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], axis=-1).astype(np.uint8).reshape(4096, 64, 64, 3)
    return rgb, R.levels(rgb, antialias=False)


@pytest.mark.parametrize("antialias", [False, True])
def test_gray_of_every_rgb_triple(all_triples, antialias):
    """All 2^24 triples as 4096 frames of 64 x 64 x 3; at 64 x 64 the resize is the identity under both settings."""
    rgb, want = all_triples
    if antialias:
        assert torch.equal(R.levels(rgb[:64], antialias=True), want[:64])   # the oracle's identity (a sample)
    levels, status, intact = _launch([rgb], antialias)
    assert intact and status.tolist() == [0]
    differ = int((levels[0] != want).sum())
    print(f"antialias={antialias}: {differ} of {want.numel()} triples differ from the oracle")
    assert differ == 0
    assert int(levels[0].reshape(-1)[-1]) == 254                            # (255, 255, 255) -> 254.9745 -> 254


# ---- 2. exact ratios, ties -----------------------------------------------------------------------------------------

def test_exact_ratio_with_ties_rounds_half_to_even():
    """256 x 128 -> 64 x 64 without antialias: every weight is 0.5, every value a multiple of 0.25."""
    rng = np.random.default_rng(SEED + 2)
    g = rng.integers(0, 256, size=(N_FRAMES, 256, 128), dtype=np.uint8)
    c = rng.integers(0, 256, size=(N_FRAMES, 256, 128, 3), dtype=np.uint8)
    levels, status, intact = _launch([g, c], False, gaps=[3, 5])
    assert intact and status.tolist() == [0, 0]
    for b, f in enumerate((g, c)):
        A, B, d = R.frontend(f, False)
        ties = float((R.tie_distance(B) == 0).double().mean())
        print(f"channels={1 if f.ndim == 3 else 3}: d {d}, exact ties {ties:.2%}")
        assert d == 0.0 and ties > 0.15
        assert torch.equal(levels[b], A)


# ---- 3. general shapes, 5. determinism --------------------------------------------------------------------------

@pytest.fixture(scope="module")
def general():
    """The seven clips, their oracle outputs under both settings and the kernel's: computed once, read by cases 3 - 5."""
    rng = np.random.default_rng(SEED)
    frames = [rng.integers(0, 256, size=(N_FRAMES, h, w, 3), dtype=np.uint8) for h, w in SHAPES]
    gaps = [1, 7, 3, 11, 5, 9, 13]                 # every clip at an odd offset
    out = {}
    for aa in (False, True):
        levels, status, intact = _launch(frames, aa, gaps=gaps)
        out[aa] = dict(levels=levels, status=status, intact=intact, oracle=[R.frontend(f, aa) for f in frames])
    return frames, gaps, out


@pytest.mark.parametrize("antialias", [False, True])
def test_general_shapes_against_the_float64_oracle(general, antialias):
    frames, _, out = general
    got = out[antialias]
    assert got["intact"], "mvn_video_frontend wrote outside its (B, n, 64, 64) levels"
    assert got["status"].tolist() == [0] * len(SHAPES)
    excluded = total = 0
    for b, (shape, (A, B, d)) in enumerate(zip(SHAPES, got["oracle"])):
        level = got["levels"][b].double()
        delta = max(8 * d, 1e-4)
        near = R.tie_distance(B) <= delta
        wrong = int((level != R.round_half_even(B))[~near].sum())
        worst = float((level - B).abs().max())
        print(f"{shape} antialias={antialias}: d {d:.3e}, delta {delta:.3e}, within delta of a tie "
              f"{float(near.double().mean()):.3%}, levels off round(B) away from ties {wrong}, max |level - B| "
              f"{worst:.6f}, differ from A {int((level != A.double()).sum())}")
        assert wrong == 0, shape
        assert worst <= 0.5 + delta, shape
        if d == 0.0:      # torch's fp32 evaluation is exact here: then so is A, ties included
            assert torch.equal(got["levels"][b], A), shape
        excluded += int(near.sum())
        total += near.numel()
    print(f"antialias={antialias}: {excluded} of {total} pixels within delta of a tie ({excluded / total:.3%})")
    assert excluded <= 0.01 * total


@pytest.mark.parametrize("antialias", [False, True])
def test_two_launches_give_the_same_bytes(general, antialias):
    frames, gaps, out = general
    again, status, intact = _launch(frames, antialias, gaps=gaps)
    assert intact and not status.any()
    assert torch.equal(again, out[antialias]["levels"])
    # ... and a clip alone, at another offset, gives the bytes it gives inside the batch
    alone, _, _ = _launch(frames[1:2], antialias, gaps=[2])
    assert torch.equal(alone[0], out[antialias]["levels"][1])


# ---- 4. descriptors ------------------------------------------------------------------------------------------------

def test_bad_descriptors_are_refused_on_the_device(general):
    """The descriptors are device data: a span past the upload, channels = 2 and H = 0 are never read through -- the
    kernel's check precedes every address it forms -- their status is non-zero and their levels are zero."""
    from movenet_amd.ops import video_clip_descriptors, video_frontend
    frames, _, out = general
    good = frames[0]                                              # (100, 150)
    h, w = good.shape[1:3]
    claimed = [good] * 4                                          # the host lists are all in range ...
    shapes = [(h, w, 3)] * 4
    desc = video_clip_descriptors(shapes, N_FRAMES, offsets=[0] * 4)
    rec = desc.view([("offset", "<i8"), ("height", "<i4"), ("width", "<i4"), ("channels", "<i4"),
                     ("reserved", "<i4")]).reshape(4)
    rec["offset"][1] = 4 * good.size - 10                         # ... the device descriptors are not: 10 bytes left
    rec["channels"][2] = 2
    rec["height"][3] = 0
    d_desc = torch.from_numpy(desc).to(DEV)
    levels, status, intact = _launch(claimed, False, descriptors=d_desc)
    assert intact
    assert status[0] == 0 and all(int(s) != 0 for s in status[1:])
    assert torch.equal(levels[0], out[False]["levels"][0])
    assert not levels[1:].any()
    pix = torch.from_numpy(np.concatenate([good.reshape(-1)] * 4)).to(DEV)
    with pytest.raises(ValueError, match="refused clip 1"):       # the default: a non-zero status raises
        video_frontend(pix, shapes, N_FRAMES, offsets=[0] * 4, descriptors=d_desc)
    for bad, match in (([(h, w, 2)], "channels"), ([(0, w, 3)], "outside"), ([(h, 4097, 3)], "outside")):
        with pytest.raises(ValueError, match=match):              # host lists are checked before any launch
            video_frontend(pix, bad, N_FRAMES)
    with pytest.raises(ValueError, match="do not lie inside"):
        video_frontend(pix, [(h, w, 3)], N_FRAMES, offsets=[pix.numel() - 10])


# ---- 6. the loader, end to end ----------------------------------------------------------------------------------

def test_loader_raw_frames_end_to_end(tmp_path, monkeypatch):
    """Three raw clips of different sizes and one pre-made clip, batch 2: Batch.video is levels / 255 for the raw
    clips, the stored array for the pre-made one.  (No model is run on the batch here: DESIGN 4.5, known issue.)"""
    import movenet_amd.dataset as D
    import movenet_amd.wavenet as W
    from movenet_amd.dataset import get_dataloader
    monkeypatch.setattr(W, "MAX_AUDIO_FRAMES", 3000)
    monkeypatch.setattr(W, "MAX_VIDEO_FRAMES", 3)
    clips = M.write_tree(tmp_path, material=M.MATERIAL[:4], valid=1, skipped=False)
    rng = np.random.default_rng(SEED + 6)
    vids = [rng.integers(0, 256, size=(7, 30, 50, 3), dtype=np.uint8),
            rng.integers(0, 256, size=(5, 100, 70), dtype=np.uint8),
            rng.random((7, 64, 64), dtype=np.float32),                       # the pre-made form
            rng.integers(0, 256, size=(4, 121, 97, 3), dtype=np.uint8)]
    for c, v in zip(clips, vids):
        np.save(c["path"][:-4] + ".npy", v)
    scale = np.float32(1.0 / 255.0)
    want = []
    for v in vids:
        at = R.subsample_indices(v.shape[0], 3)
        want.append(v[at] if v.dtype == np.float32 else R.levels(v[at]).float().numpy() * scale)
    monkeypatch.setattr(D, "VIDEO_STAGE_BYTES", 30000)    # the second batch's launch stays whole, the first is split
    ld = get_dataloader(str(tmp_path), 64, batch_size=2, use_video=True, device=DEV)
    assert [i["video_orig_dim"] for i in ld.info] == [7, 5, 0, 4]
    first = list(ld)
    assert len(first) == 2 and ld._video_status == []      # the launches' statuses were read behind the last batch
    for k, batch in enumerate(first):
        assert tuple(batch.video.shape) == (2, 3, 64, 64, 1) and batch.video.dtype == torch.float32
        assert batch.video.is_cuda and tuple(batch.audio.shape) == (2, 64, 3000)
        for j in range(2):
            assert np.array_equal(batch.video[j, ..., 0].cpu().numpy(), want[2 * k + j]), (k, j)   # to the bit
    stats = ld.cache_stats()
    assert (stats["video_hits"], stats["video_misses"], stats["video_clips"]) == (0, 3, 3)
    assert stats["video_bytes"] == 3 * 3 * 64 * 64
    # second epoch (a NEW loader, as the trainer builds one per epoch): only hits, the same tensors
    ld2 = get_dataloader(str(tmp_path), 64, batch_size=2, use_video=True, device=DEV)
    ld2.set_epoch(1)
    for b1, b2 in zip(first, ld2):
        assert torch.equal(b1.video, b2.video) and b1.filepaths == b2.filepaths
    stats = ld2.cache_stats()
    assert (stats["video_hits"], stats["video_misses"], stats["video_clips"]) == (3, 3, 3)
