"""CPU restatement of the public HiFi-GAN release's mel front end
(jik876/hifi-gan ``meldataset.mel_spectrogram``).  TEST INFRASTRUCTURE ONLY, not a test
module.  Neither the release nor librosa is installed here, so both are restated from
their published definitions:

* :func:`librosa_mel` — ``librosa.filters.mel`` (Slaney scale, Slaney norm), float64,
  stored float32; written on its own (band by band, scalar edge frequencies), not shared
  with the package's ``mel.librosa_mel_fn``;
* :func:`mel_f32` — the release's own op sequence in float32 torch;
* :func:`mel_f64` — the same with the window product in float32 (as ``torch.stft`` forms
  it), then ``numpy.fft.rfft``, magnitude, projection and log in float64.  The GPU tests
  compare against this one.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

CONFIG = dict(sampling_rate=22050, n_fft=1024, hop_size=256, win_size=1024, num_mels=80,
              fmin=0.0, fmax=8000.0)
# the release's config_v1.json, the keys the front end reads
V1_JSON = {"num_mels": 80, "n_fft": 1024, "hop_size": 256, "win_size": 1024,
           "sampling_rate": 22050, "fmin": 0, "fmax": 8000}
LOG_CLIP = np.float32(np.log(1e-5))  # the mel of digital silence


def signals(n):
    """The ``tone + noise`` / ``chirp`` pair of tests/test_gpu_mel.py::_signals."""
    g = torch.Generator().manual_seed(0)
    t = torch.arange(n) / 22050.0
    tone = 0.3 * torch.sin(2 * np.pi * 220.0 * t) + 0.2 * torch.sin(2 * np.pi * 3100.0 * t)
    noise = 0.1 * torch.randn(n, generator=g)
    chirp = 0.5 * torch.sin(2 * np.pi * (100 + 2000 * t) * t)
    return torch.stack([tone + noise, chirp])


def quiet_signal():
    """0.8 tone + 0.05 noise burst, then 1e-4-level noise, then exact zeros (8192 each)."""
    n = 8192
    g = torch.Generator().manual_seed(3)
    t = torch.arange(3 * n) / 22050.0
    wav = 0.8 * torch.sin(2 * np.pi * 440.0 * t) + 0.05 * torch.randn(3 * n, generator=g)
    wav[n:2 * n] = 1e-4 * torch.randn(n, generator=g)
    wav[2 * n:] = 0.0
    return wav


def _slaney_hz_to_mel(hz):
    if hz >= 1000.0:
        return 15.0 + math.log(hz / 1000.0) / (math.log(6.4) / 27.0)
    return 3.0 * hz / 200.0


def _slaney_mel_to_hz(mel):
    if mel >= 15.0:
        return 1000.0 * math.exp((math.log(6.4) / 27.0) * (mel - 15.0))
    return 200.0 * mel / 3.0


def librosa_mel(sr, n_fft, n_mels, fmin, fmax):
    """float32 [n_mels, n_fft//2 + 1]: triangles between consecutive Slaney-spaced edge
    frequencies, each scaled by 2 / (its width in Hz)."""
    if fmax is None:
        fmax = sr / 2.0
    n_bins = n_fft // 2 + 1
    freqs = np.linspace(0.0, sr / 2.0, n_bins)
    lo, hi = _slaney_hz_to_mel(float(fmin)), _slaney_hz_to_mel(float(fmax))
    edges = [_slaney_mel_to_hz(m) for m in np.linspace(lo, hi, n_mels + 2)]
    out = np.zeros((n_mels, n_bins), np.float64)
    for m in range(n_mels):
        left, centre, right = edges[m], edges[m + 1], edges[m + 2]
        rise = (freqs - left) / (centre - left)
        fall = (right - freqs) / (right - centre)
        out[m] = np.clip(np.minimum(rise, fall), 0.0, None) * (2.0 / (right - left))
    return out.astype(np.float32)


def _cfg(cfg):
    c = dict(CONFIG)
    c.update(cfg or {})
    if c["fmax"] is None:
        c["fmax"] = c["sampling_rate"] / 2.0
    return c


@torch.no_grad()
def mel_f32(wav, cfg=None):
    """The release's op sequence (meldataset.py mel_spectrogram), wav [B, N] float32 →
    float32 [B, num_mels, N // hop]."""
    c = _cfg(cfg)
    n_fft, hop, win = c["n_fft"], c["hop_size"], c["win_size"]
    fb = torch.from_numpy(librosa_mel(c["sampling_rate"], n_fft, c["num_mels"], c["fmin"], c["fmax"]))
    pad = (n_fft - hop) // 2
    y = F.pad(wav.unsqueeze(1), (pad, pad), mode="reflect").squeeze(1)
    spec = torch.stft(y, n_fft, hop_length=hop, win_length=win, window=torch.hann_window(win),
                      center=False, pad_mode="reflect", normalized=False, onesided=True,
                      return_complex=True)
    spec = torch.sqrt(spec.real.pow(2) + spec.imag.pow(2) + 1e-9)
    spec = torch.matmul(fb, spec)
    return torch.log(torch.clamp(spec, min=1e-5))


@torch.no_grad()
def mel_f64(wav, cfg=None):
    """The same quantity with a float64 spectrum: wav [B, N] float32 → float64 numpy
    [B, num_mels, N // hop]."""
    c = _cfg(cfg)
    n_fft, hop, win = c["n_fft"], c["hop_size"], c["win_size"]
    fb = librosa_mel(c["sampling_rate"], n_fft, c["num_mels"], c["fmin"], c["fmax"]).astype(np.float64)
    pad = (n_fft - hop) // 2
    y = F.pad(wav.unsqueeze(1), (pad, pad), mode="reflect").squeeze(1)
    w = torch.zeros(n_fft)
    left = (n_fft - win) // 2
    w[left:left + win] = torch.hann_window(win)
    n_frames = (y.shape[-1] - n_fft) // hop + 1
    idx = torch.arange(n_frames)[:, None] * hop + torch.arange(n_fft)[None]
    frames = (y[:, idx] * w).numpy().astype(np.float64)       # fp32 product, as torch.stft
    z = np.fft.rfft(frames, axis=-1)                           # [B, frames, bins]
    mag = np.sqrt(z.real ** 2 + z.imag ** 2 + 1e-9)
    mel = np.einsum("mk,bfk->bmf", fb, mag)
    return np.log(np.maximum(mel, 1e-5))
