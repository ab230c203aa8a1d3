"""CPU: the video front end's host side -- the exported entry point and its refusals before any launch, the loader's
dispatch on dtype and shape for ``<stem>.npy`` (raw uint8 frames against the pre-made 64 x 64 form), its refusals, the
frame selection on a raw clip, the unchanged pre-made path, the trainer's flags, and a self-check of the oracle
(tests/video_frontend_reference.py).  Nothing here needs a GPU: loaders are constructed and inspected, never iterated."""
import ctypes

import numpy as np
import pytest
import torch

import video_frontend_reference as R
import wav_material as M
from movenet_amd import _native as N
from movenet_amd.dataset import WavFolderLoader, get_dataloader, inspect_video_file


# ---- the C ABI ------------------------------------------------------------------------------------------------------

def test_library_exports_the_entry_point():
    lib = N.lib()
    assert hasattr(lib, "mvn_video_frontend") and "mvn_video_frontend" in N.SIGNATURES


def test_host_refusals_return_bad_arg_with_a_text_before_any_launch():
    lib = N.lib()
    buf = (ctypes.c_uint8 * 64)()     # host memory: never dereferenced, every call below returns before a launch
    p = ctypes.addressof(buf)
    good = dict(pix=p, pix_len=64, clips=p, batch=1, n_frames=1, antialias=0, levels=p, status=p)

    def call(**kw):
        a = {**good, **kw}
        return lib.mvn_video_frontend(a["pix"], a["pix_len"], a["clips"], a["batch"], a["n_frames"], a["antialias"],
                                      a["levels"], a["status"], None)

    for bad in (dict(pix=None), dict(clips=None), dict(levels=None), dict(status=None), dict(batch=-1),
                dict(n_frames=0), dict(n_frames=-3), dict(antialias=2), dict(antialias=-1)):
        lib.mvn_abi_version()
        assert call(**bad) == N.MVN_ERR_BAD_ARG, bad
        assert "mvn_video_frontend" in N.last_error() and "bad argument" in N.last_error(), bad
    assert call(batch=0) == N.MVN_OK                   # nothing to do: no launch, so no GPU needed either
    assert call(batch=0, pix=None) == N.MVN_ERR_BAD_ARG  # ... but the pointers are still checked


def test_ops_checks_its_host_lists_without_a_gpu():
    from movenet_amd.ops import video_clip_descriptors, video_frontend
    d = video_clip_descriptors([(4, 5, 3), (2, 2, 1)], 3, None)
    rec = d.view([("offset", "<i8"), ("height", "<i4"), ("width", "<i4"), ("channels", "<i4"), ("reserved", "<i4")])
    assert d.shape == (2, 6) and d.dtype == np.int32 and d.nbytes == 2 * 24
    assert rec["offset"].ravel().tolist() == [0, 3 * 4 * 5 * 3] and rec["channels"].ravel().tolist() == [3, 1]
    with pytest.raises(RuntimeError, match="no CPU path"):     # a CPU tensor is refused, not converted
        video_frontend(torch.zeros(100, dtype=torch.uint8), [(2, 2, 1)], 1)


# ---- the oracle ------------------------------------------------------------------------------------------------------

def test_oracle_gray_truncates_and_rounding_ties_go_to_even():
    white = torch.full((1, 64, 64, 3), 255, dtype=torch.uint8)
    assert int(R.gray(white).max()) == 254 == int(R.gray(white).min())      # 254.9745 truncated
    assert bool((R.levels(white) == 254).all())                             # 64 x 64: the resize is the identity
    # 2 x 2 -> one pixel means: 128 x 128 of 2 x 2 cells (a, a, a, a + 2): mean a + 0.5, an exact tie
    a = torch.arange(0, 252, 2, dtype=torch.uint8)
    cells = torch.zeros(128, 128, dtype=torch.uint8)
    cells[0::2, 0::2] = a[:64].repeat(64, 1)
    cells[0::2, 1::2] = a[:64].repeat(64, 1)
    cells[1::2, 0::2] = a[:64].repeat(64, 1)
    cells[1::2, 1::2] = a[:64].repeat(64, 1) + 2
    A, B, d = R.frontend(cells[None], antialias=False)
    assert d == 0.0 and bool((R.tie_distance(B) == 0).all())
    assert A[0, 0].tolist() == [int(v) for v in a[:64]]                      # a even: a + 0.5 goes DOWN to a
    odd = (cells.to(torch.int16) + 1).to(torch.uint8)                        # a odd: a + 0.5 goes UP to a + 1
    assert R.levels(odd[None])[0, 0].tolist() == [int(v) + 2 for v in a[:64]]
    assert R.subsample_indices(7, 3).tolist() == [0, 3, 6]


def test_oracle_fp32_against_fp64_excludes_few_pixels():
    """What the GPU test's margin rests on: on random frames the fp32 oracle deviates from the fp64 one by d, and the
    share of pixels within delta = max(8 d, 1e-4) of a rounding tie.  Without antialias every weight is a multiple of
    1 / 128 (the output side is 64), so d is 0 and a tie is EXACT or far; measured (90 x 120, seed 0): 0.2 % are exact
    ties.  With antialias d is ~4e-5 and ~0.1 % lie within delta."""
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, size=(3, 90, 120), dtype=np.uint8)
    for aa in (False, True):
        A, B, d = R.frontend(frames, aa)
        delta = max(8 * d, 1e-4)
        near = R.tie_distance(B) <= delta
        share = float(near.double().mean())
        print(f"antialias={aa}: d {d:.3e}, delta {delta:.3e}, within delta of a tie {share:.4%}")
        assert d < 1e-3 and share < 0.01
        far = ~near
        assert torch.equal(A[far].double(), torch.round(B)[far])
        if not aa:
            assert d == 0.0 and torch.equal(A.double(), torch.round(B))


# ---- the loader -------------------------------------------------------------------------------------------------------

@pytest.fixture()
def folder(tmp_path, monkeypatch):
    import movenet_amd.wavenet as W
    monkeypatch.setattr(W, "MAX_AUDIO_FRAMES", 3000)
    clips = M.write_tree(tmp_path, material=M.MATERIAL[:3], valid=1, skipped=False)
    return tmp_path, clips


def _npy(clip):
    return clip["path"][:-4] + ".npy"


def test_dispatch_on_dtype_and_shape(folder):
    root, clips = folder
    rng = np.random.default_rng(1)
    rgb = rng.integers(0, 256, size=(7, 20, 30, 3), dtype=np.uint8)
    gray = rng.integers(0, 256, size=(5, 9, 11), dtype=np.uint8)
    old = rng.random((7, 64, 64), dtype=np.float32)
    for c, v in zip(clips, (rgb, gray, old)):
        np.save(_npy(c), v)
    assert inspect_video_file(_npy(clips[0])) == (7, 20, 30, 3)
    assert inspect_video_file(_npy(clips[1])) == (5, 9, 11, 1)
    assert inspect_video_file(_npy(clips[2])) is None
    ld = WavFolderLoader(root, 64, batch_size=2, use_video=True)
    assert ld.raw_video == {0: (7, 20, 30, 3), 1: (5, 9, 11, 1)}            # a mixed folder is fine
    assert [i["video_orig_dim"] for i in ld.info] == [7, 5, 0]
    # the frame selection on a raw clip is the linspace rule: F = 7, n = 3 -> frames 0, 3, 6
    sel = ld._raw_frames(0)
    assert sel.shape == (3, 20, 30, 3) and sel.dtype == np.uint8 and np.array_equal(sel, rgb[[0, 3, 6]])
    assert np.array_equal(ld._raw_frames(1), gray[[0, 2, 4]][..., None])    # linspace(0, 4, 3)
    # the pre-made path gives the same array as before
    v = ld._video(2)
    assert v.shape == (3, 64, 64, 1) and v.dtype == np.float32 and np.array_equal(v, old[[0, 3, 6]][..., None])
    np.save(_npy(clips[2]), old[..., None])
    assert np.array_equal(WavFolderLoader(root, 64, batch_size=2, use_video=True)._video(2), v)
    stats = ld.cache_stats()
    assert {k: stats[k] for k in ("video_hits", "video_misses", "video_clips", "video_bytes")} == dict(
        video_hits=0, video_misses=0, video_clips=0, video_bytes=0)
    assert "video_hits" not in WavFolderLoader(root, 64, batch_size=2, use_video=False).cache_stats()
    with pytest.raises(RuntimeError, match="HIP"):       # no CPU path for the front end either
        next(iter(ld))


@pytest.mark.parametrize("array,match", [
    (np.zeros((4, 8, 8, 2), np.uint8), "raw uint8 frames"),        # another channel count
    (np.zeros((4, 8, 8, 1), np.uint8), "raw uint8 frames"),
    (np.zeros((8, 8), np.uint8), "raw uint8 frames"),              # another rank
    (np.zeros((2, 4, 8, 8, 3), np.uint8), "raw uint8 frames"),
    (np.zeros((0, 8, 8, 3), np.uint8), "no video frames"),         # F < 1
    (np.zeros((1, 4097, 2, 3), np.uint8), "4096"),                 # H beyond 4096
    (np.zeros((1, 2, 4097), np.uint8), "4096"),                    # W beyond 4096
    (np.zeros((4, 32, 32), np.float32), r"expected \(F, 64, 64\) or \(F, 64, 64, 1\) gray frames"),   # today's message
    (np.zeros((4, 64, 64, 3), np.float32), r"expected \(F, 64, 64\) or \(F, 64, 64, 1\) gray frames"),
])
def test_refusals_name_the_file_when_the_loader_opens_it(folder, array, match):
    root, clips = folder
    for c in clips:
        np.save(_npy(c), np.zeros((2, 64, 64), np.float32))
    np.save(_npy(clips[1]), array)
    with pytest.raises(ValueError, match=match) as e:
        WavFolderLoader(root, 64, batch_size=1, use_video=True)
    assert clips[1]["name"] + ".npy" in str(e.value)
    WavFolderLoader(root, 64, batch_size=1, use_video=False)     # without video the file is never opened


def test_loader_options_are_checked_and_reach_it_through_get_dataloader(folder):
    root, clips = folder
    for c in clips:
        np.save(_npy(c), np.zeros((2, 8, 8, 3), np.uint8))
    ld = get_dataloader(str(root), 64, batch_size=1, use_video=True)
    assert ld.video_antialias is False
    ld = get_dataloader(str(root), 64, batch_size=1, use_video=True, video_antialias=1, video_cache_bytes=1234)
    assert ld.video_antialias is True and ld.video_cache.max_bytes == 1234
    with pytest.raises(ValueError, match="video_antialias"):
        get_dataloader(str(root), 64, batch_size=1, use_video=True, video_antialias=2)
    # loaders of one split, antialias setting and device share the level cache; another setting has its own
    a = WavFolderLoader(root, 64, batch_size=1, use_video=True)
    b = WavFolderLoader(root, 64, batch_size=1, use_video=True, train=True)
    c = WavFolderLoader(root, 64, batch_size=1, use_video=True, video_antialias=True)
    assert a.video_cache is b.video_cache and a.video_cache is not c.video_cache


def test_trainer_flags_reach_get_dataloader(monkeypatch):
    import movenet_amd.pytorch_lightning_trainer as T
    from movenet_amd.config import TrainingConfig, arg_parser, config_from_args
    base = ["--dataset", "synthetic://clips=2,frames=1000", "--input_channels", "64", "--layer_size", "2",
            "--stack_size", "2"]
    cfg = config_from_args(arg_parser().parse_args(base))
    assert cfg.video_antialias is False
    cfg = config_from_args(arg_parser().parse_args(base + ["--video_antialias", "1"]))
    assert cfg.video_antialias is True
    back = TrainingConfig.from_json(cfg.to_json())
    assert back.video_antialias is True
    import json
    old = json.loads(cfg.to_json())
    del old["video_antialias"]                                  # a JSON written before the field existed
    back = TrainingConfig.from_json(json.dumps(old))
    assert back.video_antialias is False
    seen = []
    monkeypatch.setattr(T, "get_dataloader", lambda *a, **kw: seen.append(kw) or "loader")
    module = T.Dance2Music("synthetic://clips=2,frames=1000", cfg)
    assert module.train_dataloader() == "loader" and module.val_dataloader() == "loader"
    assert [(kw["video_antialias"], kw["train"]) for kw in seen] == [(True, True), (True, False)]
