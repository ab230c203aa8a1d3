"""GPU: mvn_logmel_frontend against the float64 restatement of its definition (tests/logmel_reference.py), Q = 256.

The error is taken on the mel ENERGIES, per frame, as max_m |E - E64| / max_m E64.  The yardstick is the same
expression evaluated in fp32 on the CPU by torch matmul (a direct DFT with the same fp32 tables: the same algorithm
class); the kernel may be at most 4 x as far from float64 as the yardstick is -- the 4 allows for another order of an
N-term fp32 sum and says nothing about the kernel.  Measured (yardstick / kernel, worst frame): see DESIGN 4.5d.
Where a frame lands (which frame tile, which workgroup) is also held to the bit, by translating the clip."""
import functools

import numpy as np
import pytest
import torch

import logmel_reference as R
from helpers import DEV
from movenet_amd import _native as N
from movenet_amd import ops

pytestmark = pytest.mark.gpu
Q = 256
kTile = 32   # frames per workgroup of lm_dft_kernel
SHAPES = [(3, 100, 64, 16, 8), (2, 1000, 256, 64, 20), (1, 17, 64, 64, 3), (2, 2048, 1024, 256, 80)]
# More than one frame tile of lm_dft_kernel (32 frames) and more than one workgroup of lm_mel_kernel (64 frames):
SHAPES += [
    (2, 1100, 64, 16, 8),       # F = 69: three frame tiles, the last with 5 live frames; two lm_mel workgroups
    (1, 1008, 64, 16, 5),       # F = 64 = p_ld: every tile full
    (1, 1024, 64, 16, 5),       # F = 65: one frame into a third tile and into a second lm_mel workgroup
    (1, 8448, 1024, 256, 80),   # F = 34 at the production n_fft, hop and M: two frame tiles, 17 bin tiles
]


def _indices(B, T, seed):
    """mu-law indices of uniform noise of amplitude 0.5 (every mel energy is then orders above the floor)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.5, 0.5, size=(B, T))
    mu = Q - 1.0
    y = np.sign(x) * np.log1p(mu * np.abs(x)) / np.log1p(mu)
    return np.clip(((y + 1.0) / 2.0 * mu + 0.5).astype(np.int64), 0, Q - 1).astype(np.int32)


def _tables(n_fft):
    ang = 2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft
    return (0.5 - 0.5 * np.cos(ang)).astype(np.float32), np.concatenate([np.cos(ang), np.sin(ang)]).astype(np.float32)


def _call(idx, n_fft, hop, fbank, floor=1e-5, energies=False, pad=3, fill=float("nan")):
    """The C call on NaN-filled output rows of F + pad columns -> the whole (B, M, F + pad) tensor."""
    lib = N.lib()
    B, T = idx.shape
    M, F = fbank.shape[0], T // hop + 1
    window, twiddle = (torch.from_numpy(t).to(DEV) for t in _tables(n_fft))
    fb = torch.from_numpy(np.ascontiguousarray(fbank, dtype=np.float32)).to(DEV)
    out = torch.full((B, M, F + pad), fill, dtype=torch.float32, device=DEV)
    n = lib.mvn_logmel_scratch_floats(B, T, n_fft, hop)
    scratch = torch.empty(n, dtype=torch.float32, device=DEV)
    N.check(lib.mvn_logmel_frontend(torch.from_numpy(idx).to(DEV).data_ptr(), B, T, Q, n_fft, hop, M, window.data_ptr(),
                                    twiddle.data_ptr(), fb.data_ptr(), floor, int(energies), out.data_ptr(), F + pad,
                                    scratch.data_ptr(), n, torch.cuda.current_stream(DEV).cuda_stream),
            "mvn_logmel_frontend")
    torch.cuda.synchronize()
    return out.cpu()


def _yardstick(idx, n_fft, hop, fbank):
    """The definition in fp32 on the CPU: fp32 decode, fp32 tables, torch matmul for the DFT and the filterbank."""
    mu = torch.tensor(Q - 1.0)
    y = (torch.from_numpy(idx).to(torch.float32) / mu) * 2.0 - 1.0
    x = torch.copysign((torch.exp(y.abs() * torch.log1p(mu)) - 1.0) / mu, y)
    window, twiddle = (torch.from_numpy(t) for t in _tables(n_fft))
    fr = torch.from_numpy(R.frames_of(x.numpy(), n_fft, hop)) * window          # (B, F, N) fp32
    k = np.arange(n_fft // 2 + 1)[:, None] * np.arange(n_fft)[None, :] % n_fft
    c, s = twiddle[:n_fft][k], twiddle[n_fft:][k]
    re, im = fr @ c.T, fr @ s.T
    power = re * re + im * im
    return torch.einsum("mk,bfk->bmf", torch.from_numpy(np.asarray(fbank, dtype=np.float32)), power)


def _frame_err(E, E64):
    E, E64 = np.asarray(E, dtype=np.float64), np.asarray(E64)
    return (np.abs(E - E64).max(axis=1) / E64.max(axis=1)).max()


@functools.lru_cache(maxsize=None)
def _case(shape):
    B, T, n_fft, hop, M = shape
    idx = _indices(B, T, 1000 + T)
    fbank = R.mel_filterbank(M, n_fft, 16000.0, 0.0, 8000.0)
    E64 = R.mel_energies(idx, Q, n_fft, hop, fbank)
    return idx, fbank, E64, _frame_err(_yardstick(idx, n_fft, hop, fbank).numpy(), E64)


@pytest.mark.parametrize("shape", SHAPES)
def test_energies_and_log_against_float64(shape):
    B, T, n_fft, hop, M = shape
    idx, fbank, E64, yard = _case(shape)
    F = T // hop + 1
    assert E64.shape == (B, M, F) and (E64.max(axis=1) > 1e3 * 1e-5).all()   # orders above the floor
    got = _call(idx, n_fft, hop, fbank, energies=True)
    assert bool(torch.isnan(got[:, :, F:]).all()), "columns past F were written"
    E = got[:, :, :F].numpy()
    assert np.isfinite(E).all()
    err = _frame_err(E, E64)
    print(f"logmel {shape}: energies vs float64 -- fp32 torch matmul {yard:.3e}, kernel {err:.3e}")
    assert err <= 4.0 * yard, (shape, err, yard)
    # the log output: the same energies through floor and log (logf and the fp32 energies' own error, in log units)
    lg = _call(idx, n_fft, hop, fbank)
    assert bool(torch.isnan(lg[:, :, F:]).all())
    want = np.log(np.maximum(E.astype(np.float64), 1e-5))
    assert np.abs(lg[:, :, :F].numpy() - want).max() < 1e-5 * max(1.0, np.abs(want).max())
    # ... and through the Python entry point, cached tables and all
    via = ops.logmel(torch.from_numpy(idx).to(DEV), Q, n_fft, hop, fbank)
    assert tuple(via.shape) == (B, M, F) and torch.equal(via.cpu(), lg[:, :, :F])


def test_a_frame_tile_is_a_translation_of_tile_0_to_the_bit():
    """n_fft 64, hop 16, T = 1600 (F = 101, four frame tiles): clip b is clip a moved right by 512 samples = 32 hops =
    one frame tile.  Frame j + 32 of b then has the operands of frame j of a on the same lane (j & 31) of the same waves,
    and lm_mel_kernel's sum per frame knows no position: the same bits, no tolerance."""
    B, T, n_fft, hop, M, shift = 2, 1600, 64, 16, 8, 512
    assert shift == kTile * hop
    idx_a = _indices(B, T, 1600)
    idx_b = np.concatenate([_indices(B, shift, 512), idx_a[:, :T - shift]], axis=1)
    assert idx_b.shape == idx_a.shape and not np.array_equal(idx_b[:, :shift], idx_a[:, :shift])
    fbank = R.mel_filterbank(M, n_fft, 16000.0, 0.0, 8000.0)
    F = T // hop + 1
    # frames of a whose window [16 j - 32, 16 j + 32) lies inside [0, T - 512)
    js = np.array([j for j in range(F) if j * hop - n_fft // 2 >= 0 and j * hop + n_fft // 2 <= T - shift])
    assert js[0] == 2 and js[-1] == 66 and len(js) >= 60
    to = js + kTile
    assert to[-1] < F and {int(t) // kTile for t in to} == {1, 2, 3}
    for energies in (True, False):
        a = _call(idx_a, n_fft, hop, fbank, energies=energies)[:, :, :F]
        b = _call(idx_b, n_fft, hop, fbank, energies=energies)[:, :, :F]
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
        assert torch.equal(b[:, :, to], a[:, :, js]), "a frame tile is not a translation of tile 0"
        assert not torch.equal(b[:, :, js], a[:, :, js])   # (b is another clip, not the same one)


def test_sine_on_a_bin_lands_in_its_band():
    n_fft, hop, T = 64, 16, 256
    t = np.arange(T)
    x = 0.5 * np.sin(2.0 * np.pi * 8 * t / n_fft)
    mu = Q - 1.0
    y = np.sign(x) * np.log1p(mu * np.abs(x)) / np.log1p(mu)
    idx = ((y + 1.0) / 2.0 * mu + 0.5).astype(np.int32)[None, :]
    fbank = R.mel_filterbank(6, n_fft, 16000.0, 0.0, 8000.0)
    band = int(fbank[:, 8].argmax())
    E64 = R.mel_energies(idx, Q, n_fft, hop, fbank)
    E = _call(idx, n_fft, hop, fbank, energies=True)[:, :, :T // hop + 1].numpy()
    inner = slice(2, T // hop - 1)   # frames that lie wholly inside the clip
    assert (E64[0, :, inner].argmax(axis=0) == band).all()
    assert (E[0, :, inner].argmax(axis=0) == band).all()
    assert _frame_err(E, E64) < 1e-5


def test_floor_edges_reproducibility_and_bad_indices():
    shape = SHAPES[0]
    B, T, n_fft, hop, M = shape
    idx, fbank, E64, _ = _case(shape)
    F = T // hop + 1
    # floor = 1.0 above every energy of an all-mid-class input: log(1.0f) = 0.0f exactly, everywhere
    mid = np.full((B, T), Q // 2, dtype=np.int32)
    out = _call(mid, n_fft, hop, fbank, floor=1.0)[:, :, :F]
    assert bool((out == 0.0).all()) and not bool(torch.signbit(out).any())
    # two calls: the same bits
    a, b = _call(idx, n_fft, hop, fbank), _call(idx, n_fft, hop, fbank)
    assert torch.equal(a[:, :, :F], b[:, :, :F])
    # index -1 and index Q decode as 0: the same bits as the reference with those samples at 0
    bad = idx.copy()
    bad[0, 5], bad[1, 40], bad[2, T - 1] = -1, Q, -7
    got = _call(bad, n_fft, hop, fbank, energies=True)[:, :, :F].numpy()
    assert np.isfinite(got).all()
    want = R.mel_energies(bad, Q, n_fft, hop, fbank)   # (the restatement decodes them as 0 too)
    assert _frame_err(got, want) <= 4.0 * max(_case(shape)[3], 1e-7)
    assert not np.array_equal(got, _call(idx, n_fft, hop, fbank, energies=True)[:, :, :F].numpy())
