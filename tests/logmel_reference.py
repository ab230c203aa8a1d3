"""float64 numpy restatements of the definitions of the log-mel front end and the frame up-sampler (DESIGN 4.5d,
include/movenet_hip.h), written from the definitions alone -- none of the library's code is used."""
import numpy as np


def mel_filterbank(n_mels, n_fft, rate, f_min, f_max):
    """HTK mel scale, triangles between n_mels + 2 equally spaced mel points, peak 1, no area normalisation."""
    def hz_to_mel(f):
        return 2595.0 * np.log10(1.0 + f / 700.0)

    def mel_to_hz(m):
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    pts = mel_to_hz(np.linspace(hz_to_mel(float(f_min)), hz_to_mel(float(f_max)), n_mels + 2))
    bank = np.zeros((n_mels, n_fft // 2 + 1))
    for m in range(n_mels):
        lo, mid, hi = pts[m], pts[m + 1], pts[m + 2]
        for k in range(n_fft // 2 + 1):
            f = k * rate / n_fft
            if lo < f <= mid:
                bank[m, k] = (f - lo) / (mid - lo)
            elif mid < f < hi:
                bank[m, k] = (hi - f) / (hi - mid)
    return bank


def mu_law_decode(index, classes):
    """x = sign(y) ((1 + mu)^|y| - 1) / mu with y = 2 index / mu - 1; 0 for an index outside [0, classes)."""
    q = np.asarray(index, dtype=np.int64)
    mu = float(classes - 1)
    y = q.astype(np.float64) / mu * 2.0 - 1.0
    x = np.sign(y) * (np.exp(np.abs(y) * np.log1p(mu)) - 1.0) / mu
    return np.where((q < 0) | (q >= classes), 0.0, x)


def n_frames(n_samples, hop):
    return n_samples // hop + 1


def hann(n_fft):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)


def frames_of(x, n_fft, hop):
    """(B, T) -> (B, F, N): frame j covers samples [j hop - N/2, j hop + N/2), zeros outside [0, T)."""
    B, T = x.shape
    F = n_frames(T, hop)
    padded = np.zeros((B, T + 2 * n_fft + F * hop), dtype=x.dtype)
    padded[:, n_fft:n_fft + T] = x
    starts = n_fft + np.arange(F) * hop - n_fft // 2
    return padded[:, starts[:, None] + np.arange(n_fft)[None, :]]


def dft_matrices(n_fft):
    """cos and sin of 2 pi k n / N, (N/2 + 1, N) each, float64 with the angle reduced exactly ((k n) mod N)."""
    k = np.arange(n_fft // 2 + 1)[:, None]
    n = np.arange(n_fft)[None, :]
    ang = 2.0 * np.pi * ((k * n) % n_fft) / n_fft
    return np.cos(ang), np.sin(ang)


def mel_energies(index, classes, n_fft, hop, fbank):
    """(B, T) indices -> (B, M, F) float64 mel energies, before floor and log."""
    x = mu_law_decode(index, classes)
    fr = frames_of(x, n_fft, hop) * hann(n_fft)            # (B, F, N)
    c, s = dft_matrices(n_fft)
    re, im = fr @ c.T, fr @ s.T                             # (B, F, bins)
    power = re * re + im * im
    return np.einsum("mk,bfk->bmf", np.asarray(fbank, dtype=np.float64), power)


def logmel(index, classes, n_fft, hop, fbank, floor=1e-5):
    return np.log(np.maximum(mel_energies(index, classes, n_fft, hop, fbank), floor))


def upsample_features(mel, w, bias, hop, n_samples):
    """ctx[b, c, t] = bias[c] + sum_m w[c, m] ((1 - a) mel[b, m, j] + a mel[b, m, j1]); torch (differentiable) or numpy
    inputs, in whatever precision they come."""
    import torch
    mel, w, bias = (torch.as_tensor(v) for v in (mel, w, bias))
    F = mel.shape[2]
    t = torch.arange(n_samples)
    j = t // hop
    j1 = torch.clamp(j + 1, max=F - 1)
    a = ((t % hop).to(mel.dtype) / hop)[None, None, :]
    mix = (1.0 - a) * mel[:, :, j] + a * mel[:, :, j1]
    return torch.einsum("cm,bmt->bct", w, mix) + bias[None, :, None]
