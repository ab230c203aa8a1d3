"""Batches for the trainer entry point.

The reference's loader decodes Kinetics mp4 clips (movenet/dataset.py:59-364:
torchvision.io + torchaudio + pytorchvideo), none of which exist offline; that
storage/codec side is out of scope.  What the trainer
consumes is the ``Batch`` tuple ``(audio one-hot (B,Q,T), video|None, contexts,
filepaths, info)`` (dataset.py:186-203) and that contract is kept here, fed by
a synthetic source:

    --dataset synthetic://clips=64,frames=16000,seed=1234

Class indices are U{0..Q-1} (SURVEY.md section 8d "Synthetic inputs"); the
optional random contiguous crop ``batch_subsample_frac`` follows
dataset.py:232-242.

Beside it, a folder of integer-PCM WAV files in the reference's layout (``WavFolderLoader``):

    --dataset /data/my_wavs          # <dir>/train/<context>/*.wav, <dir>/valid/<context>/*.wav

What the reference does to a decoded waveform (channel mean, resample to MAX_AUDIO_FRAMES, min-max normalisation,
mu-law, one-hot: dataset.py:253-289) runs on the GPU behind the upload (ops.audio_frontend), and so does what it does to
decoded frames (RGB -> gray, resize to 64 x 64: dataset.py:292-310; ops.video_frontend); the decoders themselves stay
out of scope.
"""
from __future__ import annotations

import math
import random
from typing import Iterator, List, Optional

import numpy as np
import torch

from .utils.weights import one_hot


class Batch:
    def __init__(self, audio, video, contexts, filepaths, info, lengths=None):
        self.audio, self.video = audio, video
        self.contexts, self.filepaths, self.info = contexts, filepaths, info
        # real samples per clip where the rows end in padding (WavFolderLoader(clip_length="native")), else None;
        # an attribute beside the five fields the batch unpacks into
        self.lengths = lengths

    def pin_memory(self):
        self.audio = self.audio.pin_memory()
        if self.video is not None:
            self.video = self.video.pin_memory()
        return self

    def __iter__(self):
        yield from (self.audio, self.video, self.contexts, self.filepaths, self.info)


def parse_synthetic(spec: str) -> dict:
    if not spec.startswith("synthetic://"):
        raise ValueError(
            f"dataset {spec!r}: only synthetic://clips=N,frames=T[,seed=S] sources are built; "
            "the Kinetics mp4 decoder of the reference is out of scope (SURVEY.md section 2)")
    out = dict(clips=8, frames=16000, seed=1234)
    body = spec[len("synthetic://"):]
    for item in filter(None, body.split(",")):
        k, v = item.split("=")
        out[k.strip()] = int(v)
    return out


class SyntheticLoader:
    """Deterministic, shardable replacement for DataLoader(KineticsDataset)."""

    def __init__(self, spec: str, input_channels: int, batch_size: int, train: bool = True,
                 rank: int = 0, world_size: int = 1, shuffle: bool = False,
                 batch_subsample_frac: Optional[float] = None, use_video: bool = False,
                 device=None, **_ignored):
        cfg = parse_synthetic(spec)
        self.n_clips, self.frames = cfg["clips"], cfg["frames"]
        self.seed = cfg["seed"] + (0 if train else 10007)
        self.Q, self.batch_size = input_channels, batch_size
        self.rank, self.world = rank, max(world_size, 1)
        self.shuffle, self.frac = shuffle, batch_subsample_frac
        self.use_video = use_video
        # device (an MI355X) given: the class indices are shipped (B x T x 4 bytes) and the one-hot
        # (B,Q,T) tensor of the Batch contract is formed THERE (mvn_index_to_onehot, row F2) --
        # a 16 x 256 x 16000 fp32 one-hot is 262 MB of PCIe traffic per batch otherwise
        self.device = torch.device(device) if device is not None else None
        if use_video and (self.frames % 1000 or batch_subsample_frac is not None):
            raise ValueError("video batches need frames % 1000 == 0 and no batch_subsample_frac "
                             "(the reference crops audio and video independently, dataset.py:232-242, "
                             "which its own size assert then rejects)")
        self.epoch = 0
        self.contexts = ["synthetic"]  # (the one context name every synthetic clip reports)

    def set_epoch(self, epoch: int) -> None:
        self.epoch = epoch

    def _order(self) -> List[int]:
        order = list(range(self.n_clips))
        if self.shuffle:
            random.Random(self.seed + self.epoch).shuffle(order)
        # DistributedSampler semantics: pad to a multiple of world, stride by rank
        per = math.ceil(len(order) / self.world)
        order = (order + order[: per * self.world - len(order)])[self.rank::self.world]
        return order

    def __len__(self) -> int:
        return math.ceil(len(self._order()) / self.batch_size)

    def _clip(self, i: int) -> np.ndarray:
        rng = np.random.default_rng(self.seed * 1000003 + i)
        return rng.integers(0, self.Q, size=self.frames, dtype=np.int64)

    def __iter__(self) -> Iterator[Batch]:
        order = self._order()
        crop_rng = random.Random(self.seed * 31 + self.epoch * 7 + self.rank)
        for s in range(0, len(order), self.batch_size):
            ids = order[s:s + self.batch_size]
            idx = np.stack([self._clip(i) for i in ids])
            if self.device is not None and self.device.type == "cuda":
                audio = _one_hot_on_device(idx, self.Q, self.device)
            else:
                audio = one_hot(torch.from_numpy(idx), self.Q)
            if self.frac is not None:
                n = math.ceil(audio.shape[-1] * self.frac)
                start = crop_rng.randint(0, audio.shape[-1] - n)
                audio = audio[..., start:start + n]
            video = None
            if self.use_video:
                # U[0,1) frames, one 64x64 gray frame per 1000 samples
                # (movenet/wavenet.py:27-31: 160 frames <-> 160000 samples)
                vr = np.random.default_rng(self.seed * 7919 + 4321 + ids[0])
                frames = vr.random((len(ids), self.frames // 1000, 64, 64, 1), dtype=np.float32)
                if self.device is not None and self.device.type == "cuda":
                    video = _to_device_async(frames, self.device)
                else:
                    video = torch.from_numpy(frames)
            yield Batch(audio, video, ["synthetic"] * len(ids),
                        [f"synthetic://{i}" for i in ids],
                        [dict(video_fps=0.0, audio_fps=float(self.frames) / 10.0)] * len(ids))


class _PinnedRing:
    """A few persistent pinned host buffers the loader stages its batches in, taken in turn; an
    event behind each asynchronous copy says when its buffer may be overwritten (polled:
    generation.wait_event).  Pinned + asynchronous: a copy from pageable memory makes the host wait
    until everything queued on the stream -- the whole previous step -- has run."""

    def __init__(self, slots: int = 4):
        self.slots, self.next = [None] * slots, 0

    def stage(self, src: np.ndarray) -> tuple:
        """``src``: a numpy array.  It is copied into the slot with numpy (one thread): a torch CPU
        op of this size opens an OpenMP region on every visible core, whose threads then spin for
        their block time -- in a container with a CPU quota that alone can exhaust the quota of a
        scheduler period and freeze the whole process for the rest of it (r3: 60-90 ms stalls at
        arbitrary places of every second or third Trainer.fit step; none in loops without per-step
        CPU tensor ops)."""
        from .generation import wait_event
        i, self.next = self.next, (self.next + 1) % len(self.slots)
        slot = self.slots[i]
        dtype = torch.from_numpy(np.empty(0, dtype=src.dtype)).dtype
        if slot is None or tuple(slot[0].shape) != src.shape or slot[0].dtype != dtype:
            slot = self.slots[i] = [torch.empty(src.shape, dtype=dtype).pin_memory(), None]
        if slot[1] is not None:
            wait_event(slot[1])
        np.copyto(slot[0].numpy(), src)
        return slot

    @staticmethod
    def to_device(slot, device: torch.device) -> torch.Tensor:
        """Asynchronous copy on the CURRENT stream (pinned source: the host does not wait)."""
        out = slot[0].to(device, non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record(torch.cuda.current_stream(device))
        return out


_RINGS: dict = {}


def _ring(kind: str, device: torch.device) -> _PinnedRing:
    key = (kind, device.index)
    if key not in _RINGS:
        _RINGS[key] = _PinnedRing()
    return _RINGS[key]


def _one_hot_on_device(idx: np.ndarray, Q: int, device: torch.device) -> torch.Tensor:
    """(B,T) integer host indices (numpy) -> (B,Q,T) fp32 one-hot on ``device`` through the C ABI (row F2).

    The indices (4 bytes per sample) cross PCIe from a persistent pinned staging buffer as an
    asynchronous copy on the training stream, which then expands them itself
    (mvn_index_to_onehot: ~70 us for 16 x 256 x 16000).  A copy from pageable memory would make
    the host wait until everything queued on that stream -- the whole previous step -- has run."""
    from . import _native as N
    B, T = idx.shape
    with torch.cuda.device(device):
        d_idx = _PinnedRing.to_device(_ring("idx", device).stage(np.ascontiguousarray(idx, dtype=np.int32)), device)
        out = torch.empty(B, Q, T, dtype=torch.float32, device=device)
        N.check(N.lib().mvn_index_to_onehot(d_idx.data_ptr(), d_idx.stride(0), out.data_ptr(), B, Q, T,
                                            torch.cuda.current_stream(device).cuda_stream), "mvn_index_to_onehot")
    return out


def _to_device_async(x: np.ndarray, device: torch.device) -> torch.Tensor:
    """Host array -> device through the pinned staging ring (see _one_hot_on_device)."""
    with torch.cuda.device(device):
        return _PinnedRing.to_device(_ring("video", device).stage(np.ascontiguousarray(x)), device)


def _upload_pcm(device: torch.device, parts: list, kind: str, desc: np.ndarray, least: int = 0) -> tuple:
    """A batch's int16 ``parts`` back to back in ONE upload (at least ``least`` samples of it) and its descriptor array
    ``desc``, through the pinned rings "pcm" and ``kind`` -> (PCM, descriptors) on the device."""
    total = sum(p.size for p in parts)
    # (padded to a 256 Ki-sample step: batches of like-sized clips reuse the ring's pinned buffers)
    pcm = np.zeros(-(-max(total, least) // (1 << 18)) * (1 << 18), dtype=np.int16)
    np.concatenate(parts, out=pcm[:total])
    d_pcm = _PinnedRing.to_device(_ring("pcm", device).stage(pcm), device)
    return d_pcm, _PinnedRing.to_device(_ring(kind, device).stage(desc), device)


def read_wav_header(path: str) -> dict:
    """rate / frames / channels / sample width of an integer-PCM WAV (standard library ``wave``); ValueError naming
    the file for anything else (float WAVs, compressed formats, broken headers)."""
    import wave
    try:
        with wave.open(str(path), "rb") as w:
            info = dict(rate=w.getframerate(), frames=w.getnframes(), channels=w.getnchannels(),
                        width=w.getsampwidth(), comptype=w.getcomptype())
    except (wave.Error, EOFError) as e:
        raise ValueError(f"{path}: not an integer-PCM WAV ({e})") from e
    if info["comptype"] != "NONE" or info["width"] not in (1, 2, 3, 4) or info["channels"] < 1:
        raise ValueError(f"{path}: only 8/16/24/32-bit integer PCM is read "
                         f"(sample width {info['width']}, compression {info['comptype']})")
    return info


def read_wav_pcm16(path: str) -> tuple:
    """(interleaved int16 samples, frames, channels, rate) of an integer-PCM WAV, in the form the GPU front end
    takes: 16-bit as stored; 8-bit (unsigned) as ``(v - 128) << 8``, which is the same waveform exactly; 24- and
    32-bit rounded to the nearest 16-bit value (saturating) -- the model quantises to at most 256 classes."""
    import wave
    h = read_wav_header(path)
    with wave.open(str(path), "rb") as w:
        raw = w.readframes(h["frames"])
    pcm, n = _pcm16_of(raw, h["width"], h["channels"])
    return pcm, n, h["channels"], h["rate"]


def read_wav_span(path: str, first: int, frames: int, header: Optional[dict] = None) -> tuple:
    """``read_wav_pcm16`` of the frames [first, first + frames) alone (``wave.setpos`` / ``readframes``: nothing else of
    the file is read): (interleaved int16 samples, frames read, channels, rate), the same 8/16/24/32-bit handling.
    The span is clipped to the file."""
    import wave
    h = read_wav_header(path) if header is None else header
    first = min(max(int(first), 0), h["frames"])
    frames = min(max(int(frames), 0), h["frames"] - first)
    with wave.open(str(path), "rb") as w:
        w.setpos(first)
        raw = w.readframes(frames)
    pcm, n = _pcm16_of(raw, h["width"], h["channels"])
    return pcm, n, h["channels"], h["rate"]


def _pcm16_of(raw: bytes, width: int, ch: int) -> tuple:
    """(interleaved int16 samples, whole frames) of a WAV's data bytes at ``width`` bytes per sample."""
    n = len(raw) // (width * ch)
    raw = raw[: n * width * ch]
    if width == 2:
        pcm = np.frombuffer(raw, dtype="<i2")
    elif width == 1:
        pcm = (np.frombuffer(raw, dtype=np.uint8).astype(np.int16) - 128) << 8
    else:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, width).astype(np.int64)
        v = sum(b[:, k] << (8 * k) for k in range(width))
        v = np.where(v >= 1 << (8 * width - 1), v - (1 << (8 * width)), v)  # two's complement
        shift = 8 * width - 16
        pcm = np.clip((v + (1 << (shift - 1))) >> shift, -32768, 32767)
    return np.ascontiguousarray(pcm, dtype=np.int16), n


FILE_RANGE_CHUNK = 1 << 20  # frames per read of wav_file_range


def wav_file_range(path: str, header: Optional[dict] = None) -> tuple:
    """(lo, hi) of a file's channel-mean PCM / 32768, as float32 numbers formed the way the front end forms them (the
    integer channel sum over fp32(32768 channels)); the file is read FILE_RANGE_CHUNK frames at a time."""
    h = read_wav_header(path) if header is None else header
    lo = hi = None
    for first in range(0, h["frames"], FILE_RANGE_CHUNK):
        pcm, n, ch, _ = read_wav_span(path, first, FILE_RANGE_CHUNK, header=h)
        if n < 1:
            break
        sums = pcm.reshape(n, ch).sum(axis=1, dtype=np.int64)
        lo = int(sums.min()) if lo is None else min(lo, int(sums.min()))
        hi = int(sums.max()) if hi is None else max(hi, int(sums.max()))
    if lo is None:
        return 0.0, 0.0
    den = np.float32(32768.0) * np.float32(h["channels"])
    return float(np.float32(lo) / den), float(np.float32(hi) / den)


def window_geometry(rate: int, audio_rate: int) -> tuple:
    """(orig, new, W) of the resample from ``rate`` to ``audio_rate``: the reduced ratio and how far the taps of one
    output reach, i0 - W .. i0 + W + 1 -- the front end's own numbers (csrc/audio.hip: af_geom_taps)."""
    g = math.gcd(int(rate), int(audio_rate))
    orig, new = int(rate) // g, int(audio_rate) // g
    s = 0.99 * min(orig, new) / orig
    return orig, new, int(6.0 / s) + 1


def resampled_frames(file_frames: int, rate: int, audio_rate: int) -> int:
    """n_file = ceil(file_frames new / orig): the outputs a whole file resamples to."""
    orig, new, _ = window_geometry(rate, audio_rate)
    return -(-int(file_frames) * new // orig)


class _IndexCache:
    """(N,) int16 class indices of the clips seen so far, on the device.  They do not depend on the epoch (the crop
    does).  Past ``max_bytes`` nothing is evicted: new clips are simply not kept."""

    def __init__(self, max_bytes: int):
        self.max_bytes, self.bytes = int(max_bytes), 0
        self.rows: dict = {}
        self.lengths: dict = {}  # clip -> real samples of its row (by-rate rows end in silence), beside the indices
        self.ranges: dict = {}  # file -> (lo, hi) of its channel mean (clip_length="window", window_gain="file")
        self.hits = self.misses = 0

    def put(self, key, row: torch.Tensor, length: Optional[int] = None) -> None:
        size = row.numel() * 2
        if key not in self.rows and self.bytes + size <= self.max_bytes:
            self.rows[key] = row.to(torch.int16)
            self.lengths[key] = row.numel() if length is None else int(length)
            self.bytes += size


_INDEX_CACHES: dict = {}


class _LevelCache:
    """(n, 64, 64) uint8 gray levels of the raw-frame clips seen so far, on the device: one byte per pixel.  Past ``max_bytes`` nothing is evicted: new clips are simply not kept."""

    def __init__(self, max_bytes: int):
        self.max_bytes, self.bytes = int(max_bytes), 0
        self.rows: dict = {}
        self.hits = self.misses = 0

    def put(self, key, levels: torch.Tensor) -> None:
        size = levels.numel()
        if key not in self.rows and self.bytes + size <= self.max_bytes:
            self.rows[key] = levels.clone()  # (a view of the launch's output would keep the whole batch alive)
            self.bytes += size


_LEVEL_CACHES: dict = {}

# Bound on the selected frames one front-end launch takes (and so on a pinned staging buffer of the ring): a batch whose
# raw frames exceed it is split over several launches, clip by clip; a single clip beyond it goes up alone.
VIDEO_STAGE_BYTES = 256 << 20
VIDEO_UNIT_SCALE = float(np.float32(1.0 / 255.0))  # levels -> the [0, 1] of the pre-made form


def inspect_video_file(fp: str):
    """What ``<stem>.npy`` holds, from its header (the array is memory-mapped, nothing is read): ``None`` for the
    pre-made form -- (F, 64, 64) or (F, 64, 64, 1), not uint8, taken as is -- or (F, H, W, channels) for raw uint8
    frames, (F, H, W, 3) RGB or (F, H, W) gray.  ValueError naming the file for anything else."""
    v = np.load(fp, mmap_mode="r", allow_pickle=False)
    if v.dtype != np.uint8:
        shape = v.shape[:-1] if v.ndim == 4 and v.shape[-1] == 1 else v.shape
        if len(shape) != 3 or shape[1:] != (64, 64) or shape[0] < 1:
            raise ValueError(f"{fp}: expected (F, 64, 64) or (F, 64, 64, 1) gray frames, got {v.shape}")
        return None
    if not (v.ndim == 3 or (v.ndim == 4 and v.shape[-1] == 3)):
        raise ValueError(f"{fp}: raw uint8 frames are (F, H, W, 3) RGB or (F, H, W) gray, got {v.shape}")
    F, H, W = (int(x) for x in v.shape[:3])
    if F < 1:
        raise ValueError(f"{fp}: no video frames in {v.shape}")
    if not (1 <= H <= 4096 and 1 <= W <= 4096):
        raise ValueError(f"{fp}: frames of {H} x {W} lie outside 1 .. 4096 per side")
    return F, H, W, (3 if v.ndim == 4 else 1)


class WavFolderLoader:
    """Clips from a folder of WAV files, in the reference's KineticsDataset layout with ``.wav`` for ``.mp4``
    (movenet/dataset.py:101-140):

        <dir>/train/<context>/*.wav      <dir>/valid/<context>/*.wav

    Stems containing ``_raw`` or starting with ``.`` are skipped (:126).  Same interface and sharding rules as
    SyntheticLoader.  The files are read with the standard library's ``wave`` (integer PCM only); the interleaved
    int16 samples of a batch cross PCIe from the pinned staging ring as one asynchronous copy on the training stream,
    and everything the reference does to a decoded waveform -- channel mean, resample of the whole clip to
    MAX_AUDIO_FRAMES, min-max normalisation, mu-law (dataset.py:253-289) -- runs behind it on the GPU
    (ops.audio_frontend), then the one-hot expansion of the Batch contract (mvn_index_to_onehot).  ``__iter__`` never
    waits for the GPU.  There is no CPU path: iterating needs ``device=`` to be an MI355X.

    Build definitions (torchaudio is absent, so these are stated, not pinned): the resample is
    ``sinc_interp_hann`` with ``lowpass_filter_width = 6``, ``rolloff = 0.99``; of the reference's ``sum() == 0``
    test before normalising, only the silent-clip case is reproduced -- a clip with ``max == min`` is left as it is.

    Index cache: the (N,) indices of every clip seen stay on the device as int16, up to ``cache_bytes``; from the
    second epoch on a cached clip costs no file read, no upload and no front-end launch.  Loaders of the same split,
    class count, normalisation and device share one cache (the trainer builds a loader per epoch).

    Video (``use_video=True``): ``<stem>.npy`` beside ``<stem>.wav``, reduced to ``frames // 1000`` frames by
    pytorchvideo's uniform_temporal_subsample rule.  Two forms, told apart by dtype, which may be mixed in a folder:

    * pre-made: (F, 64, 64) or (F, 64, 64, 1), not uint8, values in [0, 1], ALREADY gray and ALREADY 64 x 64, taken as
      they are;
    * raw frames, as a decoder hands them over: uint8 (F, H, W, 3) RGB or (F, H, W) gray, H and W in [1, 4096].  The
      file is memory-mapped and only the selected frames are copied out; the selected frames of a batch cross PCIe as
      one asynchronous copy with their descriptors, and the reference's ``resize_video`` (torchvision
      rgb_to_grayscale, then resize to 64 x 64: dataset.py:292-310) runs behind it on the GPU (ops.video_frontend;
      ``video_antialias`` False is torchvision 0.13 - 0.16's resize of a tensor, True the default of 0.17 on).  A
      batch whose selected frames exceed VIDEO_STAGE_BYTES is split over several launches.  The uint8 levels of every
      raw clip seen stay on the device up to ``video_cache_bytes``, shared by loaders of the same split, antialias
      setting and device; a cached clip costs no file read, no upload and no launch.  ``Batch.video`` is
      ``levels.float() * fp32(1 / 255)``: the [0, 1] of the pre-made form.  (The reference's loader hands its model
      0 .. 255; that range is not offered.)  The kernel's per-clip status of every launch is read once, when the
      epoch's last batch has been handed out, and a refusal raises there: iterating itself never waits for the GPU.

    Clips of their own length (``clip_length="native"``; the default ``"resample"`` is the rule above, to
    the bit): every clip is resampled to ONE rate, ``audio_rate``, instead of onto one width -- clip b comes out
    ``n_b = min(frames, round(frames_b * audio_rate / rate_b))`` samples long (``native_plan``), a clip that would come
    out longer contributes its head, the first ``ceil(frames * rate_b / audio_rate)`` source frames resampled to
    ``frames`` -- into rows of the unchanged width ``frames`` with silence behind it (ops.audio_frontend_var), and
    ``Batch.lengths`` says how many samples of each row are real; the index cache keeps the lengths beside the
    indices.  With ``batch_subsample_frac`` the window is drawn as above and a clip's length inside it is
    ``clamp(len_b - start, 0, n)``.  Refused with ``use_video`` (video batches are fixed at ``frames``).

    Random windows of long files (``clip_length="window"``): a row is ``frames`` consecutive samples of
    a file's resample to ``audio_rate``, starting at ``out_first``; only the source frames those samples' taps reach are
    read from disk (``read_wav_span``) and uploaded (``window_plan``), and ops.audio_frontend_window forms the row --
    the bits the whole file's resample has at those columns.  File i, ``n_file_i`` samples long at ``audio_rate``,
    has ``max(1, ceil(n_file_i / frames))`` windows per epoch, so an epoch covers the corpus once in expectation;
    sharding and shuffling are the rules above applied to (file, window) pairs.  Training windows start at a draw
    from U{0 .. max(0, n_file - frames)} keyed on (seed, epoch, file, window) alone -- not on rank, batch size or
    order -- and pass the index cache by; validation windows tile the file (window w starts at ``w * frames``, the
    last one is short) and are cached by (file, window).  ``Batch.lengths`` carries every row's real samples and
    ``info`` rows the window's ``out_first``.  ``window_gain="file"`` (the default) normalises every window by the
    (min, max) of its whole file's channel mean, found on the host in bounded chunks when the file is first touched;
    ``"window"`` by the window's own.  Refused with ``use_video``; a file's length is not limited.

    ``preemphasis=a`` (0 < a < 1; 0, the default, leaves every call above as it is), fixed per loader: whichever
    front-end form the loader uses quantises the pre-emphasised row (vn[k] - a vn[k-1]) / (1 + a) of the normalised
    waveform, a row's first column without a predecessor (``ops.audio_frontend``), in all three ``clip_length`` modes.
    The index cache then holds emphasised classes, in a cache of its own per coefficient."""

    @staticmethod
    def native_plan(clip_frames: int, clip_rate: int, frames: int, audio_rate: int):
        """(source frames read, samples they are resampled to) of one clip under ``clip_length="native"``."""
        n = int(round(clip_frames * audio_rate / clip_rate))
        if n > frames:
            return min(int(clip_frames), int(math.ceil(frames * clip_rate / audio_rate))), int(frames)
        return int(clip_frames), max(n, 1)

    @staticmethod
    def window_plan(file_frames: int, rate: int, frames: int, audio_rate: int, out_first: int):
        """(span_first, span_frames, n_out) of the window of ``frames`` samples at ``out_first`` of a file's resample to
        ``audio_rate``: n_out = min(frames, n_file - out_first) samples, formed from the source frames
        [i0(out_first) - W, i0(out_first + n_out - 1) + W + 1] clipped to the file, i0(j) = j orig // new."""
        orig, new, W = window_geometry(rate, audio_rate)
        n_file = -(-int(file_frames) * new // orig)
        if not 0 <= out_first < n_file:
            raise ValueError(f"out_first {out_first} lies outside the file's {n_file} samples")
        n_out = min(int(frames), n_file - int(out_first))
        first = max(0, int(out_first) * orig // new - W)
        last = min(int(file_frames) - 1, (int(out_first) + n_out - 1) * orig // new + W + 1)
        return first, last - first + 1, n_out

    @staticmethod
    def window_count(file_frames: int, rate: int, frames: int, audio_rate: int) -> int:
        """Windows of one file per epoch: max(1, ceil(n_file / frames))."""
        return max(1, -(-resampled_frames(file_frames, rate, audio_rate) // int(frames)))

    def window_start(self, file: int, window: int) -> int:
        """``out_first`` of (file, window) in this epoch: validation windows tile the file; a training window is drawn
        from U{0 .. max(0, n_file - frames)} by a generator keyed on (seed, epoch, file, window)."""
        if not self.train:
            return window * self.frames
        key = ((self.seed * 1000003 + self.epoch) * 1000003 + file) * 1000003 + window
        return random.Random(key).randint(0, max(0, self.n_file[file] - self.frames))

    @staticmethod
    def cropped_lengths(lengths, start: int, n: int):
        """Lengths of the clips inside the window [start, start + n) of their rows."""
        return [min(max(int(v) - start, 0), n) for v in lengths]

    def __init__(self, root, input_channels: int, batch_size: int, train: bool = True,
                 rank: int = 0, world_size: int = 1, shuffle: bool = False,
                 batch_subsample_frac: Optional[float] = None, use_video: bool = False,
                 normalize_audio: bool = True, device=None, cache_bytes: int = 4 << 30,
                 video_antialias: bool = False, video_cache_bytes: int = 4 << 30,
                 clip_length: str = "resample", audio_rate: int = 16000, window_gain: str = "file",
                 preemphasis: float = 0.0, **_ignored):
        import os
        from pathlib import Path
        from . import wavenet as W
        self.root_path = Path(root) / ("train" if train else "valid")
        self.frames = int(W.MAX_AUDIO_FRAMES)
        self.seed = 1234 + (0 if train else 10007)
        self.Q, self.batch_size = input_channels, batch_size
        self.rank, self.world = rank, max(world_size, 1)
        self.shuffle, self.frac = shuffle, batch_subsample_frac
        self.use_video, self.normalize = use_video, bool(normalize_audio)
        self.device = torch.device(device) if device is not None else None
        if use_video and (self.frames % 1000 or batch_subsample_frac is not None):
            raise ValueError("video batches need frames % 1000 == 0 and no batch_subsample_frac "
                             "(the reference crops audio and video independently, dataset.py:232-242, "
                             "which its own size assert then rejects)")
        if clip_length not in ("resample", "native", "window"):
            raise ValueError(f"clip_length must be 'resample', 'native' or 'window', got {clip_length!r}")
        if window_gain not in ("file", "window"):
            raise ValueError(f"window_gain must be 'file' or 'window', got {window_gain!r}")
        if isinstance(audio_rate, bool) or not isinstance(audio_rate, int) or audio_rate < 1:
            raise ValueError(f"audio_rate must be a positive integer, got {audio_rate!r}")
        self.native, self.audio_rate = clip_length == "native", int(audio_rate)
        self.window, self.window_gain, self.train = clip_length == "window", window_gain, bool(train)
        if (self.native or self.window) and use_video:
            raise ValueError(f"clip_length={clip_length!r} cannot be combined with use_video: video batches are fixed at "
                             f"{self.frames} frames")
        if input_channels > 32768:
            raise ValueError("input_channels above 32768 do not fit the int16 index cache")
        if video_antialias not in (False, True, 0, 1):
            raise ValueError(f"video_antialias must be 0 or 1, got {video_antialias!r}")
        self.video_antialias = bool(video_antialias)
        from ._native import emphasis
        emphasis(preemphasis)  # ValueError outside [0, 1)
        self.preemphasis = float(preemphasis)
        # (what the front-end calls get: nothing at 0, so that they are the calls they were)
        self._emph = {"preemphasis": self.preemphasis} if self.preemphasis > 0.0 else {}
        self._video_status: list = []  # (clips, status tensor) of the front-end launches not yet looked at
        self.raw_video: dict = {}  # clip -> (F, H, W, channels) of a raw-frame file (pre-made files are absent)
        self.contexts = _context_folders(self.root_path)
        self.index = []  # (context, path, header)
        for context in self.contexts:
            for fp in sorted((self.root_path / context).glob("*.wav")):
                if "_raw" in fp.stem or fp.stem.startswith("."):
                    continue
                h = read_wav_header(str(fp))
                if h["frames"] < 1:
                    raise ValueError(f"{fp}: no audio frames")
                if (self.native or self.window) and h["rate"] > 100 * self.audio_rate:
                    raise ValueError(f"{fp}: a rate of {h['rate']} Hz is more than 100 x audio_rate {self.audio_rate}")
                if not (self.native or self.window) and h["frames"] > 100 * self.frames:
                    raise ValueError(f"{fp}: {h['frames']} frames is more than 100 x the {self.frames} frames "
                                     "the front end resamples to")
                if use_video and not fp.with_suffix(".npy").is_file():
                    raise ValueError(f"{fp}: use_video needs the clip's frames in {fp.with_suffix('.npy').name}")
                if use_video:
                    raw = inspect_video_file(str(fp.with_suffix(".npy")))
                    if raw is not None:
                        self.raw_video[len(self.index)] = raw
                self.index.append((context, str(fp), h))
        if not self.index:
            raise ValueError(f"{self.root_path}: no .wav clips (expected <context>/*.wav below it)")
        self.filepaths = [fp for _, fp, _ in self.index]
        self.info = [dict(video_fps=0.0, audio_fps=float(h["rate"]),
                          video_orig_dim=self.raw_video[i][0] if i in self.raw_video else 0,
                          audio_orig_dim=int(h["frames"])) for i, (_, _, h) in enumerate(self.index)]
        self.n_clips = len(self.index)
        key = (os.path.abspath(str(self.root_path)), self.Q, self.frames, self.normalize, str(self.device))
        if self.native:  # (by-rate rows are other rows: a cache of their own per rate)
            key += ("native", self.audio_rate)
        if self.window:
            key += ("window", self.audio_rate, self.window_gain)
            # an epoch's rows are (file, window) pairs; _order shuffles and shards their numbers
            self.n_file = [resampled_frames(h["frames"], h["rate"], self.audio_rate) for _, _, h in self.index]
            self.pairs = [(i, w) for i, (_, _, h) in enumerate(self.index)
                          for w in range(self.window_count(h["frames"], h["rate"], self.frames, self.audio_rate))]
            self.n_clips = len(self.pairs)
        if self._emph:  # (emphasised classes are other rows: a cache of their own per coefficient)
            key += ("preemphasis", self.preemphasis)
        self.plans = [self.native_plan(h["frames"], h["rate"], self.frames, self.audio_rate) if self.native
                      else (int(h["frames"]), self.frames) for _, _, h in self.index]
        cache = _INDEX_CACHES.get(key)
        if cache is None or cache.max_bytes != int(cache_bytes):
            cache = _INDEX_CACHES[key] = _IndexCache(cache_bytes)
        self.cache = cache
        vkey = (os.path.abspath(str(self.root_path)), self.frames, self.video_antialias, str(self.device))
        vcache = _LEVEL_CACHES.get(vkey)
        if vcache is None or vcache.max_bytes != int(video_cache_bytes):
            vcache = _LEVEL_CACHES[vkey] = _LevelCache(video_cache_bytes)
        self.video_cache = vcache
        self.epoch = 0

    set_epoch = SyntheticLoader.set_epoch
    _order = SyntheticLoader._order
    __len__ = SyntheticLoader.__len__

    def cache_stats(self) -> dict:
        c = self.cache
        stats = dict(hits=c.hits, misses=c.misses, clips=len(c.rows), bytes=c.bytes)
        if self.use_video:  # the raw-frame clips' level cache (pre-made clips pass it by)
            v = self.video_cache
            stats.update(video_hits=v.hits, video_misses=v.misses, video_clips=len(v.rows), video_bytes=v.bytes)
        return stats

    def _frame_selection(self, F: int) -> np.ndarray:
        """pytorchvideo.transforms.functional.uniform_temporal_subsample: linspace, clamp, truncate."""
        return np.clip(np.linspace(0, F - 1, self.frames // 1000), 0, F - 1).astype(np.int64)

    def _raw_frames(self, i: int, out: Optional[np.ndarray] = None) -> np.ndarray:
        """The selected frames of raw clip ``i`` as (n, H, W, channels) uint8, copied out of the memory-mapped file
        (the frames that are not selected are never read)."""
        F, H, W, ch = self.raw_video[i]
        v = np.load(self.index[i][1][:-len(".wav")] + ".npy", mmap_mode="r", allow_pickle=False)
        at = self._frame_selection(F)
        if out is None:
            out = np.empty((len(at), H, W, ch), dtype=np.uint8)
        # (mode="clip": the default "raise" gathers into a temporary first; the indices are in range by construction)
        np.take(v.reshape(F, H, W, ch), at, axis=0, out=out.reshape(len(at), H, W, ch), mode="clip")
        return out

    def _levels(self, ids: List[int]) -> dict:
        """clip -> (n, 64, 64) uint8 levels on the device for the raw clips among ``ids``: cached ones as they are,
        the others read, uploaded and sent through the front end, one launch per VIDEO_STAGE_BYTES of frames."""
        from .ops import video_clip_descriptors, video_frontend
        cache, dev, n = self.video_cache, self.device, self.frames // 1000
        raw = [i for i in ids if i in self.raw_video]
        todo = [i for i in dict.fromkeys(raw) if i not in cache.rows]
        cache.hits += sum(i in cache.rows for i in raw)
        cache.misses += len(raw) - sum(i in cache.rows for i in raw)
        got = {i: cache.rows[i] for i in raw if i in cache.rows}
        size = lambda i: n * self.raw_video[i][1] * self.raw_video[i][2] * self.raw_video[i][3]
        while todo:
            group = [todo.pop(0)]
            total = size(group[0])
            while todo and total + size(todo[0]) <= VIDEO_STAGE_BYTES:
                total += size(todo[0])
                group.append(todo.pop(0))
            # (padded to a 1 MiB step: batches of like-sized clips reuse the ring's pinned buffers)
            pix = np.empty(-(-total // (1 << 20)) * (1 << 20), dtype=np.uint8)
            at = 0
            for i in group:
                self._raw_frames(i, out=pix[at:at + size(i)])
                at += size(i)
            shapes = [self.raw_video[i][1:] for i in group]
            d_pix = _PinnedRing.to_device(_ring("pix", dev).stage(pix), dev)
            d_desc = _PinnedRing.to_device(_ring("vclips", dev).stage(video_clip_descriptors(shapes, n)), dev)
            levels, status = video_frontend(d_pix, shapes, n, antialias=self.video_antialias, descriptors=d_desc,
                                            return_status=True)
            self._video_status.append((list(group), status))
            for row, i in enumerate(group):
                got[i] = levels[row]
                cache.put(i, levels[row])
        return got

    def check_video_status(self) -> None:
        """Reads the per-clip status of the front-end launches made so far (this waits for them) and raises ValueError
        naming the file of a clip the kernel refused.  ``__iter__`` calls it behind the epoch's last batch."""
        pending, self._video_status = self._video_status, []
        for group, status in pending:
            for i, st in zip(group, status.cpu().tolist()):
                if st:
                    raise ValueError(f"{self.index[i][1][:-len('.wav')]}.npy: the video front end refused the clip "
                                     f"on the device (status {st})")

    def _video_batch(self, ids: List[int]) -> torch.Tensor:
        """(B, n, 64, 64, 1) float32 on the device: raw clips through the front end, scaled into [0, 1];
        pre-made clips as they are."""
        dev = self.device
        if not any(i in self.raw_video for i in ids):
            return _to_device_async(np.stack([self._video(i) for i in ids]), dev)
        with torch.cuda.device(dev):
            levels = self._levels(ids)
            rows = {i: levels[i].to(torch.float32) * VIDEO_UNIT_SCALE for i in dict.fromkeys(ids) if i in levels}
            made = [i for i in dict.fromkeys(ids) if i not in levels]
            if made:
                up = _to_device_async(np.stack([self._video(i) for i in made]), dev)
                rows.update({i: up[k, ..., 0] for k, i in enumerate(made)})
            return torch.stack([rows[i] for i in ids])[..., None]

    def _video(self, i: int) -> np.ndarray:
        """The selected frames of a pre-made clip, (n, 64, 64, 1) float32 as stored."""
        fp = self.index[i][1][:-len(".wav")] + ".npy"
        v = np.load(fp, allow_pickle=False)
        if v.ndim == 4 and v.shape[-1] == 1:
            v = v[..., 0]
        if v.ndim != 3 or v.shape[1:] != (64, 64) or v.shape[0] < 1:
            raise ValueError(f"{fp}: expected (F, 64, 64) or (F, 64, 64, 1) gray frames, got {v.shape}")
        return np.ascontiguousarray(v[self._frame_selection(v.shape[0])], dtype=np.float32)[..., None]

    def _indices(self, ids: List[int]) -> torch.Tensor:
        """(B, N) int32 class indices of the clips on the device: cached rows as they are, the others read,
        uploaded and sent through the front end in ONE launch pair."""
        from .ops import audio_clip_descriptors, audio_clip_var_descriptors, audio_frontend, audio_frontend_var
        cache, dev = self.cache, self.device
        todo = [i for i in dict.fromkeys(ids) if i not in cache.rows]
        cache.hits += sum(i in cache.rows for i in ids)
        cache.misses += len(ids) - sum(i in cache.rows for i in ids)
        fresh = {}
        if todo:
            clips = [read_wav_pcm16(self.index[i][1]) for i in todo]
            if self.native:  # a clip that would come out longer than the row contributes its head
                clips = [(c[0].reshape(-1)[:self.plans[i][0] * c[2]], self.plans[i][0], c[2])
                         for i, c in zip(todo, clips)]
            pcm, frames, channels = [c[0] for c in clips], [c[1] for c in clips], [c[2] for c in clips]
            if self.native:
                d_pcm, d_desc = _upload_pcm(dev, pcm, "clips_var", audio_clip_var_descriptors(
                    frames, channels, [self.plans[i][1] for i in todo]))
                idx = audio_frontend_var(d_pcm, d_desc, self.Q, self.frames, normalize=self.normalize, **self._emph)
            else:
                d_pcm, d_desc = _upload_pcm(dev, pcm, "clips", audio_clip_descriptors(frames, channels))
                idx = audio_frontend(d_pcm, frames, channels, self.Q, n_out=self.frames, normalize=self.normalize,
                                     descriptors=d_desc, **self._emph)
            for row, i in enumerate(todo):
                fresh[i] = idx[row]
                cache.put(i, idx[row], self.plans[i][1])
        if len(todo) == len(ids) and todo == list(ids):
            return idx
        return torch.stack([fresh[i] if i in fresh else cache.rows[i].to(torch.int32) for i in ids])

    def file_range(self, file: int) -> tuple:
        """(lo, hi) the windows of ``file`` are normalised by: its channel mean's (min, max) under window_gain="file"
        (found once per loader cache), (0, 0) -- the window's own -- otherwise."""
        if self.window_gain != "file":
            return 0.0, 0.0
        ranges = self.cache.ranges
        if file not in ranges:
            ranges[file] = wav_file_range(self.index[file][1], header=self.index[file][2])
        return ranges[file]

    def _window_indices(self, rows: list) -> tuple:
        """``rows``: (file, window, out_first) per row -> ((B, frames) int32 class indices on the device, lengths).
        Validation windows come from and go to the index cache, keyed (file, window); of the others only the spans
        their taps reach are read and uploaded, and ONE launch pair forms them."""
        from .ops import audio_clip_window_descriptors, audio_frontend_window
        cache, dev = self.cache, self.device
        keys = [(i, w) for i, w, _ in rows]
        cached = [not self.train and k in cache.rows for k in keys]
        if not self.train:
            cache.hits += sum(cached)
            cache.misses += len(rows) - sum(cached)
        todo, plans = [], []
        for (i, w, out_first), hit in zip(rows, cached):
            if not hit and (self.train or (i, w) not in [(a, b) for a, b, _ in todo]):
                h = self.index[i][2]
                todo.append((i, w, out_first))
                plans.append(self.window_plan(h["frames"], h["rate"], self.frames, self.audio_rate, out_first))
        fresh, idx = [], None
        if todo:
            spans = [read_wav_span(self.index[i][1], p[0], p[1], header=self.index[i][2])
                     for (i, _, _), p in zip(todo, plans)]
            for (i, _, _), p, sp in zip(todo, plans, spans):
                if sp[1] != p[1]:
                    raise ValueError(f"{self.index[i][1]}: {sp[1]} of the {p[1]} frames at {p[0]} could be read")
            ranges = [self.file_range(i) for i, _, _ in todo]
            desc = audio_clip_window_descriptors(
                [p[0] for p in plans], [p[1] for p in plans], [self.index[i][2]["frames"] for i, _, _ in todo],
                [sp[2] for sp in spans], [o for _, _, o in todo], [p[2] for p in plans],
                [self.index[i][2]["rate"] for i, _, _ in todo], self.audio_rate,
                lo=[r[0] for r in ranges], hi=[r[1] for r in ranges])
            d_pcm, d_desc = _upload_pcm(dev, [sp[0] for sp in spans], "clips_window", desc, least=1)
            idx = audio_frontend_window(d_pcm, d_desc, self.Q, self.frames, normalize=self.normalize,
                                        **self._emph)
            for row, ((i, w, _), p) in enumerate(zip(todo, plans)):
                fresh.append(((i, w), idx[row], p[2]))
                if not self.train:
                    cache.put((i, w), idx[row], p[2])
        if len(todo) == len(rows):
            return idx, [p[2] for p in plans]
        made = {k: (row, n) for k, row, n in fresh}
        out = [made[k] if k in made else (cache.rows[k].to(torch.int32), cache.lengths[k]) for k in keys]
        return torch.stack([r for r, _ in out]), [n for _, n in out]

    def __iter__(self) -> Iterator[Batch]:
        if self.device is None or self.device.type != "cuda":
            raise RuntimeError("WavFolderLoader: the waveform front end is a HIP kernel; pass device= an MI355X "
                               "(there is no CPU path)")
        from . import _native as N
        order = self._order()
        crop_rng = random.Random(self.seed * 31 + self.epoch * 7 + self.rank)
        dev = self.device
        for s in range(0, len(order), self.batch_size):
            ids = order[s:s + self.batch_size]
            info = None
            with torch.cuda.device(dev):
                if self.window:  # the order's numbers are (file, window) pairs; from here on `ids` are their files
                    rows = [self.pairs[k] + (self.window_start(*self.pairs[k]),) for k in ids]
                    idx, lengths = self._window_indices(rows)
                    ids = [i for i, _, _ in rows]
                    info = [dict(self.info[i], out_first=o) for i, _, o in rows]
                else:
                    idx = self._indices(ids)
                    lengths = [self.cache.lengths.get(i, self.plans[i][1]) for i in ids] if self.native else None
                B, T = idx.shape
                if self.frac is not None:  # dataset.py:232-237, on the indices: only the crop is expanded
                    n = math.ceil(T * self.frac)
                    start = crop_rng.randint(0, T - n)
                    idx, T = idx[:, start:start + n], n
                    if lengths is not None:
                        lengths = self.cropped_lengths(lengths, start, n)
                audio = torch.empty(B, self.Q, T, dtype=torch.float32, device=dev)
                N.check(N.lib().mvn_index_to_onehot(idx.data_ptr(), idx.stride(0), audio.data_ptr(), B, self.Q, T,
                                                    torch.cuda.current_stream(dev).cuda_stream),
                        "mvn_index_to_onehot")
            video = None
            if self.use_video:
                video = self._video_batch(ids)
            yield Batch(audio, video, [self.index[i][0] for i in ids], [self.filepaths[i] for i in ids],
                        [self.info[i] for i in ids] if info is None else info, lengths=lengths)
        self.check_video_status()


def _is_wav_folder(filepath) -> bool:
    import os
    p = str(filepath)
    return os.path.isdir(p) and (os.path.isdir(os.path.join(p, "train")) or os.path.isdir(os.path.join(p, "valid")))


def _context_folders(split_path) -> List[str]:
    """Sorted names of the <context> folders below one split of a WAV tree (no file is opened)."""
    from pathlib import Path
    split_path = Path(split_path)
    return sorted(p.name for p in split_path.glob("*") if p.is_dir()) if split_path.is_dir() else []


def training_contexts(filepath) -> List[str]:
    """The context names of a source's TRAINING split, sorted -- the class map of ``--use_global`` -- without building
    a loader: the <context> folders of ``<dir>/train``, or the one name every synthetic clip reports."""
    import os
    if not str(filepath).startswith("synthetic://") and _is_wav_folder(filepath):
        return _context_folders(os.path.join(str(filepath), "train"))
    parse_synthetic(str(filepath))  # (ValueError for a source that is neither)
    return ["synthetic"]


def get_dataloader(filepath, input_channels: int, batch_size: int = 64, train: bool = True,
                   rank: int = 0, world_size: int = 0, use_video: bool = True,
                   normalize_audio: bool = True, batch_subsample_frac: Optional[float] = None,
                   **kwargs):
    """Signature of movenet/dataset.py:59-98.  ``synthetic://...`` gives a SyntheticLoader; an existing directory
    with a ``train`` or ``valid`` sub-folder gives a WavFolderLoader; anything else raises ValueError."""
    if not str(filepath).startswith("synthetic://") and _is_wav_folder(filepath):
        extra = {k: kwargs[k] for k in ("cache_bytes", "video_antialias", "video_cache_bytes", "clip_length",
                                        "audio_rate", "window_gain", "preemphasis") if k in kwargs}
        return WavFolderLoader(filepath, input_channels, batch_size, train=train, rank=rank,
                               world_size=world_size, shuffle=kwargs.get("shuffle", False),
                               batch_subsample_frac=batch_subsample_frac, use_video=use_video,
                               normalize_audio=normalize_audio, device=kwargs.get("device"), **extra)
    return SyntheticLoader(str(filepath), input_channels, batch_size, train=train, rank=rank,
                           world_size=world_size, shuffle=kwargs.get("shuffle", False),
                           batch_subsample_frac=batch_subsample_frac, use_video=use_video,
                           device=kwargs.get("device"))


# -- mu-law companding: the formula the project states (RESEARCH.md:156-163).
# The reference calls torchaudio.functional.mu_law_encoding/decoding, which is
# absent offline and pinned by no fixture in the reference => PARITY UNPINNED.
def mu_law_encoding(x: torch.Tensor, quantization_channels: int) -> torch.Tensor:
    mu = quantization_channels - 1.0
    x = x.to(torch.float32)
    y = torch.sign(x) * torch.log1p(mu * torch.abs(x)) / math.log1p(mu)
    return ((y + 1) / 2 * mu + 0.5).to(torch.int64)


def mu_law_decoding(q: torch.Tensor, quantization_channels: int) -> torch.Tensor:
    mu = quantization_channels - 1.0
    y = (q.to(torch.float32) / mu) * 2 - 1.0
    return torch.sign(y) * (torch.exp(torch.abs(y) * math.log1p(mu)) - 1.0) / mu
