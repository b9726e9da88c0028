"""CPU float64 restatement of the spectral distances (csrc/spectral_distance.hip).  TEST
INFRASTRUCTURE ONLY, not a test module.

* :func:`stft_logmag64` — ``ln(|STFT x| + eps)`` as ``torch.stft(center=True, reflect,
  hann_window(win))`` frames it: the window product in float32 (as torch.stft forms it), then
  ``numpy.fft.rfft``, magnitude and log in float64;
* :func:`stft_distance64` — per item (Σ|d|, Σd², frames) of two signals at one resolution;
* :func:`sums64` — the same two sums of any two arrays, formed in float64;
* :func:`inputs` — the shared signals ``a`` and ``b``.

Mel distances take their mels from ``release_mel_oracle.mel_f64`` and
``oracle.mel_torch.log_mel64``.
"""
import numpy as np
import torch

from release_mel_oracle import signals

RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))
EPS = 1e-5
N = 8269


def inputs(n=N):
    """a = [tone + noise, chirp, their mean] of release_mel_oracle.signals(n), float32 [3, n];
    b = 0.9 a + 0.01 randn (generator seed 7)."""
    s = signals(n)
    a = torch.stack([s[0], s[1], 0.5 * (s[0] + s[1])])
    g = torch.Generator().manual_seed(7)
    b = 0.9 * a + 0.01 * torch.randn(a.shape, generator=g)
    return a, b


def stft_logmag64(x, n_fft, hop, win, eps=EPS):
    """x [n] float32 (n > n_fft / 2) → float64 [n // hop + 1, n_fft // 2 + 1]."""
    pad = n_fft // 2
    y = torch.nn.functional.pad(x[None, None], (pad, pad), mode="reflect")[0, 0]
    w = torch.zeros(n_fft)
    left = (n_fft - win) // 2
    w[left:left + win] = torch.hann_window(win)
    n_frames = x.numel() // hop + 1
    idx = torch.arange(n_frames)[:, None] * hop + torch.arange(n_fft)[None]
    frames = (y[idx] * w).numpy().astype(np.float64)     # fp32 product, as torch.stft
    return np.log(np.abs(np.fft.rfft(frames, axis=-1)) + eps)


def sums64(u, v):
    d = np.asarray(u, np.float64) - np.asarray(v, np.float64)
    return float(np.abs(d).sum()), float((d * d).sum())


def stft_distance64(a, b, n_fft, hop, win, lengths=None, eps=EPS):
    """a, b [B, n] float32 → (sum_abs [B], sum_sq [B], frames [B]); an item of at most
    n_fft / 2 samples has no frame."""
    B, n = a.shape
    lens = [n] * B if lengths is None else list(lengths)
    s1, s2, fr = np.zeros(B), np.zeros(B), np.zeros(B, np.int64)
    for i, m in enumerate(lens):
        if m <= n_fft // 2:
            continue
        la = stft_logmag64(a[i, :m], n_fft, hop, win, eps)
        lb = stft_logmag64(b[i, :m], n_fft, hop, win, eps)
        s1[i], s2[i] = sums64(la, lb)
        fr[i] = la.shape[0]
    return s1, s2, fr


def means(s1, s2, frames, rows):
    """(per-item l1, per-item l2, batch l1, batch l2) as metrics.SpectralDistance forms them."""
    per = rows * np.maximum(frames, 1)
    tot = rows * max(int(frames.sum()), 1)
    return s1 / per, s2 / per, s1.sum() / tot, s2.sum() / tot
