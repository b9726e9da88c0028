"""On-device log-mel framing, the vocoder's input.

Mirrors ``data/audio_processing.py``:

* :func:`extract_mel` (:31-139) — same signature, shape contract (``[time]`` or
  ``[channels, time]`` → ``[n_mels, time // hop + 1]``), resampling when
  ``sample_rate`` differs from the config's (:81-88), mono by channel mean (:93-94),
  ``log(mel + 1e-10)`` in base 10, e or a custom base (:121-133), and the
  ``debug.print_shapes`` lines (:58-59, 77-78, 89-90, 95-96, 118-119, 135-137).
* :func:`extract_mel_from_file` (:142-164), :func:`save_mel` / :func:`load_mel`
  (:167-200), :func:`load_config` (:16-28).

The arithmetic runs in the HIP kernels of ``libhifigan_hip.so``: one launch of an
FFT with a float64 spectrum + mel projection + log (:class:`MelSpectrogram`, the batched
``[B, N] → [B, n_mels, N // hop + 1]`` form that feeds ``HiFiGANGenerator``), and the
polyphase sinc resampler (:class:`Resample`, torchaudio ``Resample`` defaults).
:class:`ReleaseMelSpectrogram` is the public HiFi-GAN release's ``mel_spectrogram``
(``center=False`` framing, ``ln`` of the clipped magnitude mel, librosa's filterbank from
:func:`librosa_mel_fn`; ragged batches), the mel its checkpoints expect.
There is no CPU fallback: a CPU waveform raises.
"""
from __future__ import annotations

import ctypes
from pathlib import Path
from typing import Optional, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._frontend import (HandleOwner, check, default_device, float_ptr, lengths as _lengths,
                        ptr as _ptr, riff_chunks, stream as _stream)
from .hifigan import _lengths_on


def _log_base_code(log_base):
    """audio_processing.py:125-133: 10 / "10" → log10, "e" / math.e → ln, else custom."""
    if log_base == 10.0 or log_base == "10":
        return 10, 10.0
    if log_base == "e" or log_base == 2.718281828459045:
        return 0, 0.0
    return 1, float(log_base)


# torchaudio.functional.melscale_fbanks / _hz_to_mel / _mel_to_hz, evaluated with the same
# float32 torch ops (the reference's MelSpectrogram builds its filterbank this way,
# audio_processing.py:99-110), so the device tables are bitwise the reference's
def _hz_to_mel(freq: float, mel_scale: str) -> float:
    import math
    if mel_scale == "htk":
        return 2595.0 * math.log10(1.0 + freq / 700.0)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    mels = freq / f_sp
    if freq >= min_log_hz:
        mels = min_log_hz / f_sp + math.log(freq / min_log_hz) / (math.log(6.4) / 27.0)
    return mels


def _mel_to_hz(mels: torch.Tensor, mel_scale: str) -> torch.Tensor:
    import math
    if mel_scale == "htk":
        return 700.0 * (10.0 ** (mels / 2595.0) - 1.0)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    freqs = f_sp * mels
    min_log_mel = min_log_hz / f_sp
    logstep = math.log(6.4) / 27.0
    log_t = mels >= min_log_mel
    freqs[log_t] = min_log_hz * torch.exp(logstep * (mels[log_t] - min_log_mel))
    return freqs


def melscale_fbanks(n_freqs: int, f_min: float, f_max: float, n_mels: int, sample_rate: int,
                    norm: Optional[str], mel_scale: str) -> torch.Tensor:
    """[n_freqs, n_mels] float32 triangular filterbank (torchaudio's algorithm)."""
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs)
    m_pts = torch.linspace(_hz_to_mel(f_min, mel_scale), _hz_to_mel(f_max, mel_scale), n_mels + 2)
    f_pts = _mel_to_hz(m_pts, mel_scale)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down = (-1.0 * slopes[:, :-2]) / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    fb = torch.max(torch.zeros(1), torch.min(down, up))
    if norm == "slaney":
        fb *= (2.0 / (f_pts[2:n_mels + 2] - f_pts[:n_mels])).unsqueeze(0)
    return fb


def stft_window(n_fft: int, win_length: int) -> torch.Tensor:
    """torch.stft's effective window: torch.hann_window(win_length) (periodic, float32)
    zero-padded to n_fft, centred."""
    w = torch.zeros(n_fft)
    left = (n_fft - win_length) // 2
    w[left:left + win_length] = torch.hann_window(win_length)
    return w


class MelSpectrogram(HandleOwner):
    """torchaudio.transforms.MelSpectrogram(power=2) + log on the HIP device."""

    def __init__(self, sample_rate: int = 22050, n_fft: int = 1024, hop_length: int = 256,
                 win_length: int = 1024, n_mels: int = 80, f_min: float = 0.0,
                 f_max: float = 8000.0, mel_scale: str = "slaney", norm: Optional[str] = "slaney",
                 log_eps: float = 1e-10, log_base=10.0, device=None):
        c = _lib.HfgMelConfig()
        c.sample_rate, c.n_fft, c.hop_length, c.win_length, c.n_mels = (
            sample_rate, n_fft, hop_length, win_length, n_mels)
        c.f_min, c.f_max = f_min, f_max
        c.mel_scale = {"slaney": 0, "htk": 1}[mel_scale]
        c.norm = 1 if norm == "slaney" else 0
        c.log_eps = log_eps
        c.log_base, c.log_base_value = _log_base_code(log_base)
        self.cfg = c
        self.hop = hop_length
        self.n_mels = n_mels
        self.sample_rate = sample_rate
        self._open("hfg_mel_create", "hfg_mel_destroy", ctypes.byref(c), device=device)
        # the reference's float32 window and filterbank (bitwise torch.stft / torchaudio)
        self._window = stft_window(n_fft, win_length).contiguous()
        self._fb = melscale_fbanks(n_fft // 2 + 1, float(f_min), float(f_max), n_mels,
                                   sample_rate, norm, mel_scale).contiguous()
        if not hasattr(self.lib, "hfg_mel_set_tables"):
            # only an A/B against an older library (HFG_ALLOW_OLD_LIB=1) gets here: its
            # device tables are double-evaluated, not torchaudio's float32 ones
            import warnings
            warnings.warn("libhifigan_hip.so lacks hfg_mel_set_tables: mel tables are "
                          "double-evaluated, not the reference's float32 window / filterbank")
            return
        check(self.lib, self.lib.hfg_mel_set_tables(self.ptr, float_ptr(self._window),
                                                    float_ptr(self._fb)))

    def filterbank(self) -> torch.Tensor:
        """The [n_fft/2+1, n_mels] filterbank the device uses (torchaudio's, float32)."""
        return self._fb.clone()

    def window(self) -> torch.Tensor:
        """The [n_fft] window the device uses (torch.hann_window(win_length), centred)."""
        return self._window.clone()

    def frames(self, n_samples: int) -> int:
        return n_samples // self.hop + 1

    def __call__(self, wav: torch.Tensor) -> torch.Tensor:
        """wav [B, N] float32 on the HIP device → log-mel [B, n_mels, N//hop + 1]."""
        if not wav.is_cuda:
            raise RuntimeError("MelSpectrogram (MI355X) needs a HIP tensor; no CPU fallback")
        if wav.dim() != 2:
            raise RuntimeError("expected wav [B, N]")
        wav = wav.detach().to(torch.float32).contiguous()
        B, N = wav.shape
        T = self.frames(N)
        mel = torch.empty(B, self.n_mels, T, device=wav.device, dtype=torch.float32)
        ws_bytes = int(self.lib.hfg_mel_workspace_bytes(self.ptr, B, N))
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=wav.device)
        check(self.lib, self.lib.hfg_mel_forward(self.ptr, _ptr(wav), B, N, _ptr(mel), _ptr(ws),
                                                 ws_bytes, _stream(wav.device)))
        return mel


def librosa_mel_fn(sr: int, n_fft: int, n_mels: int, fmin: float, fmax: Optional[float]
                   ) -> np.ndarray:
    """``librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax)`` (Slaney scale, Slaney norm) as
    the release's ``meldataset.py`` calls it: float32 ``[n_mels, n_fft // 2 + 1]``, evaluated
    in float64 from the published definition (librosa is not a dependency)."""
    if fmax is None:
        fmax = sr / 2.0
    fftfreqs = np.linspace(0.0, sr / 2.0, 1 + n_fft // 2)

    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0

    def hz_to_mel(f):
        return min_log_mel + np.log(f / min_log_hz) / logstep if f >= min_log_hz else f / f_sp

    mels = np.linspace(hz_to_mel(float(fmin)), hz_to_mel(float(fmax)), n_mels + 2)
    mel_f = np.where(mels >= min_log_mel, min_log_hz * np.exp(logstep * (mels - min_log_mel)),
                     f_sp * mels)                       # mel_frequencies(n_mels + 2)
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    weights = np.zeros((n_mels, 1 + n_fft // 2))
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        weights[i] = np.maximum(0.0, np.minimum(lower, upper))
    weights *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
    return weights.astype(np.float32)


class ReleaseMelSpectrogram(HandleOwner):
    """The public HiFi-GAN release's ``meldataset.mel_spectrogram`` on the HIP device (the
    mel every released ``generator_v*`` checkpoint expects): reflect pad of
    ``(n_fft - hop_size) / 2`` a side, ``torch.stft(center=False)`` with the periodic Hann
    window, ``sqrt(re² + im² + 1e-9)``, the librosa filterbank, ``ln(max(mel, 1e-5))``.
    ``wav [B, N]`` → ``mel [B, num_mels, N // hop_size]`` in one launch (release_mel_fft,
    float64 spectrum).  :class:`MelSpectrogram` is the reference's torchaudio framing, a
    different quantity (one frame more, log10 of power).

    ``n_fft`` must be a power of two >= 16 and ``n_fft - hop_size`` even; anything else is
    refused by the constructor.  With ``lengths`` (valid samples per item of a padded batch)
    item b is framed as if it were alone with ``lengths[b]`` samples, its columns past
    ``lengths[b] // hop_size`` hold ``ln(1e-5)`` (the mel of silence), samples past its length
    are never read, and the call also returns the frame counts as a device int32 tensor —
    ready to be the Generator's ``lengths``.  There is no CPU fallback."""

    def __init__(self, sampling_rate: int = 22050, n_fft: int = 1024, hop_size: int = 256,
                 win_size: int = 1024, num_mels: int = 80, fmin: float = 0.0,
                 fmax: Optional[float] = 8000.0, device=None):
        c = _lib.HfgRelmelConfig()
        c.sampling_rate, c.n_fft, c.hop_size, c.win_size, c.num_mels = (
            int(sampling_rate), int(n_fft), int(hop_size), int(win_size), int(num_mels))
        c.fmin = float(fmin)
        c.fmax = 0.0 if fmax is None else float(fmax)   # 0: sampling_rate / 2 (config null)
        self.cfg = c
        self.sampling_rate, self.n_fft, self.hop_size = int(sampling_rate), int(n_fft), int(hop_size)
        self.win_size, self.num_mels = int(win_size), int(num_mels)
        self.pad = (self.n_fft - self.hop_size) // 2
        self._open("hfg_relmel_create", "hfg_relmel_destroy", ctypes.byref(c), device=device)
        # the release's float32 window (torch.hann_window, centred by torch.stft) and
        # librosa's filterbank, stored [n_fft/2+1, num_mels] as the kernel reads it
        self._window = stft_window(self.n_fft, self.win_size).contiguous()
        self._fb = torch.from_numpy(np.ascontiguousarray(
            librosa_mel_fn(self.sampling_rate, self.n_fft, self.num_mels, fmin, fmax).T))
        check(self.lib, self.lib.hfg_relmel_set_tables(self.ptr, float_ptr(self._window),
                                                       float_ptr(self._fb)))

    def filterbank(self) -> torch.Tensor:
        """The [n_fft/2+1, num_mels] filterbank the device uses (librosa's, transposed)."""
        return self._fb.clone()

    def window(self) -> torch.Tensor:
        """The [n_fft] window the device uses (torch.hann_window(win_size), centred)."""
        return self._window.clone()

    def frames(self, n_samples: int) -> int:
        """Frames of an n_samples item: n // hop_size, or -1 when it has none (n <= the
        reflect pad, or n < hop_size)."""
        return int(self.lib.hfg_relmel_frames(self.ptr, int(n_samples)))

    def __call__(self, wav: torch.Tensor, lengths=None):
        """wav [B, N] float32 on the HIP device → mel [B, num_mels, N // hop_size]; with
        ``lengths`` (sequence of ints or an int tensor, [B]) → (mel, frame_lengths int32 [B]
        on the device).  Host lengths are validated here; a device tensor is not read back
        (the kernel clamps it into [0, N])."""
        if not wav.is_cuda:
            raise RuntimeError("ReleaseMelSpectrogram (MI355X) needs a HIP tensor; no CPU fallback")
        if wav.dim() != 2:
            raise RuntimeError("expected wav [B, N]")
        B, N = wav.shape
        T = self.frames(N)
        if B == 0 or T < 1:
            raise RuntimeError(f"wav [{B}, {N}] has no frame: N must exceed the reflect pad "
                               f"{self.pad} and be at least hop_size {self.hop_size}")
        lens_t = None
        if lengths is not None:
            on_device = isinstance(lengths, torch.Tensor) and lengths.is_cuda
            if not on_device:
                host = torch.as_tensor(lengths)
                if host.shape != (B,):
                    raise RuntimeError(f"lengths must have shape [{B}]")
                if any(self.frames(int(n)) < 1 or int(n) > N for n in host.tolist()):
                    raise RuntimeError(f"every length must be in ({self.pad}, {N}] and at "
                                       f"least hop_size {self.hop_size}, got {host.tolist()}")
            lens_t = _lengths_on(lengths, wav.device)
            if lens_t.shape != (B,):
                raise RuntimeError(f"lengths must have shape [{B}]")
        wav = wav.detach().to(torch.float32).contiguous()
        mel = torch.empty(B, self.num_mels, T, device=wav.device, dtype=torch.float32)
        frame_lens = (torch.empty(B, device=wav.device, dtype=torch.int32)
                      if lens_t is not None else None)
        with torch.cuda.device(wav.device):
            check(self.lib, self.lib.hfg_relmel_forward(
                self.ptr, _ptr(wav), B, N, _ptr(lens_t), _ptr(mel), _ptr(frame_lens),
                _stream(wav.device)))
        return mel if lens_t is None else (mel, frame_lens)


class Resample(HandleOwner):
    """torchaudio.transforms.Resample(orig_freq, new_freq) with its defaults
    (resampling_method="sinc_interp_hann", lowpass_filter_width=6, rolloff=0.99) on the
    HIP device: ``[..., time]`` → ``[..., ceil(time * new / orig)]``.  The kernel table
    is torchaudio's ``_get_sinc_resample_kernel`` (float64, stored fp32), built by
    ``hfg_resample_kernel``; the polyphase convolution runs in ``resample_sinc``.
    :meth:`ragged` is the batched front of the release chain: padded multi-channel int16 or
    float32 items, each resampled at its own length and mixed down to mono, in one launch
    (``resample_ragged``).  Equal rates are accepted: ``__call__`` returns its input,
    ``ragged`` runs the identity filter."""

    def __init__(self, orig_freq: int = 16000, new_freq: int = 16000,
                 resampling_method: str = "sinc_interp_hann", lowpass_filter_width: int = 6,
                 rolloff: float = 0.99, beta: Optional[float] = None, *, device=None):
        if resampling_method != "sinc_interp_hann":
            raise NotImplementedError("only sinc_interp_hann (torchaudio's default, the one "
                                      "audio_processing.py:84-87 uses) is implemented")
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        self.lowpass_filter_width, self.rolloff = int(lowpass_filter_width), float(rolloff)
        self._open("hfg_resample_create", "hfg_resample_destroy", self.orig_freq, self.new_freq,
                   self.lowpass_filter_width, self.rolloff, device=device)

    def kernel(self) -> Tuple[torch.Tensor, int]:
        """(kernel [new/g, 2*width + orig/g], width) — torchaudio's (kernel, width)."""
        w, n, k = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        check(self.lib, self.lib.hfg_resample_kernel(
            self.orig_freq, self.new_freq, self.lowpass_filter_width, self.rolloff, None,
            ctypes.byref(w), ctypes.byref(n), ctypes.byref(k)))
        out = torch.zeros(n.value, k.value)
        check(self.lib, self.lib.hfg_resample_kernel(
            self.orig_freq, self.new_freq, self.lowpass_filter_width, self.rolloff,
            float_ptr(out), None, None, None))
        return out, w.value

    def out_len(self, n: int) -> int:
        return int(self.lib.hfg_resample_out_len(self.ptr, int(n)))

    def __call__(self, waveform: torch.Tensor) -> torch.Tensor:
        if not waveform.is_cuda:
            raise RuntimeError("Resample (MI355X) needs a HIP tensor; no CPU fallback")
        if self.orig_freq == self.new_freq:
            return waveform
        shape = waveform.shape
        x = waveform.detach().to(torch.float32).reshape(-1, shape[-1]).contiguous()
        B, n = x.shape
        y = torch.empty(B, self.out_len(n), device=x.device, dtype=torch.float32)
        check(self.lib, self.lib.hfg_resample_forward(self.ptr, _ptr(x), B, n, _ptr(y),
                                                      _stream(x.device)))
        return y.reshape(shape[:-1] + (y.shape[-1],))

    def ragged(self, wav: torch.Tensor, lengths=None):
        """A padded batch to mono at the new rate in one launch (``hfg_resample_ragged``):
        wav ``[B, N]`` or ``[B, C, N]`` (planar channels, C <= 8), int16 or float32, on the HIP
        device → ``(y float32 [B, out_len(N)], out_lengths int32 [B] on the device)``.  Item b is
        resampled as if cropped to ``lengths[b]`` (bitwise ``self(wav[b, :lengths[b]])`` for one
        channel; int16 enters as ``s / 32768``), channels are averaged after resampling
        (``((r_0 + r_1) + ...) / C`` in float32, the reference's ``torch.mean(dim=0)`` of the
        resampled channels), ``y[b]`` is 0 from ``out_lengths[b] = ceil(lengths[b] * new / orig)``
        on, and samples past a length are never read.  ``lengths``: None (every item has N), a
        sequence of ints or an int tensor ``[B]``; host values are validated, a device tensor is
        never read back (the kernel clamps it into ``[0, N]``).  Equal rates run the identity
        filter: ``y`` is the masked mono mix (for one channel ``wav`` itself, −0.0 becoming +0.0),
        where ``__call__`` returns its input.  There is no CPU fallback."""
        if not (isinstance(wav, torch.Tensor) and wav.is_cuda):
            raise RuntimeError("Resample.ragged (MI355X) needs a HIP tensor; no CPU fallback")
        if wav.dim() not in (2, 3) or min(wav.shape) < 1:
            raise RuntimeError(f"Resample.ragged: expected wav [B, N] or [B, C, N] with every "
                               f"dimension >= 1, got {tuple(wav.shape)}")
        if wav.dtype not in (torch.int16, torch.float32):
            raise RuntimeError(f"Resample.ragged: expected torch.int16 or torch.float32, got "
                               f"{wav.dtype}")
        B, N = wav.shape[0], wav.shape[-1]
        C = wav.shape[1] if wav.dim() == 3 else 1
        if C > _lib.RESAMPLE_MAX_CHANNELS:
            raise RuntimeError(f"Resample.ragged: at most {_lib.RESAMPLE_MAX_CHANNELS} channels, "
                               f"got {C}")
        lens_t = _lengths(lengths, B, N, wav.device)
        wav = wav.detach().contiguous()
        y = torch.empty(B, self.out_len(N), device=wav.device, dtype=torch.float32)
        out_lens = torch.empty(B, device=wav.device, dtype=torch.int32)
        with torch.cuda.device(wav.device):
            check(self.lib, self.lib.hfg_resample_ragged(
                self.ptr, _ptr(wav),
                _lib.PCM_DTYPES["int16" if wav.dtype == torch.int16 else "float32"], B, C, N,
                _ptr(lens_t), _ptr(y), _ptr(out_lens), _stream(wav.device)))
        return y, out_lens


def load_config(config_path: str = "configs/config.yaml") -> dict:
    """data/audio_processing.py:16-28"""
    import yaml
    with open(config_path, "r", encoding="utf-8") as f:
        return yaml.safe_load(f)


_EXTRACTORS = {}
_RESAMPLERS = {}


def extract_mel(waveform: torch.Tensor, sample_rate: Optional[int] = None,
                config: Optional[dict] = None, config_path: str = "configs/config.yaml"
                ) -> torch.Tensor:
    """data/audio_processing.py:31-139 on the HIP device: [time] or [channels, time]
    → log-mel [n_mels, time // hop + 1] (after resampling to the config's rate)."""
    if config is None:
        config = load_config(config_path)
    a = config["audio"]
    print_shapes = config.get("debug", {}).get("print_shapes", False)
    target_sr = a["sample_rate"]
    log_base = a.get("log_base", 10.0)
    if waveform.dim() == 1:
        waveform = waveform.unsqueeze(0)
    if print_shapes:
        print(f"[extract_mel] Input waveform shape: {waveform.shape}")
    if sample_rate is not None and sample_rate != target_sr:
        if print_shapes:
            print(f"[extract_mel] Resampling from {sample_rate}Hz to {target_sr}Hz")
        key = (int(sample_rate), int(target_sr), waveform.device)
        rs = _RESAMPLERS.get(key)
        if rs is None:
            rs = _RESAMPLERS[key] = Resample(sample_rate, target_sr, device=waveform.device)
        waveform = rs(waveform)
        if print_shapes:
            print(f"[extract_mel] Resampled waveform shape: {waveform.shape}")
    if waveform.size(0) > 1:
        waveform = torch.mean(waveform, dim=0, keepdim=True)
        if print_shapes:
            print(f"[extract_mel] Converted to mono, shape: {waveform.shape}")
    key = (target_sr, a["n_fft"], a["hop_length"], a["win_length"], a["n_mels"],
           a["fmin"], a["fmax"], a.get("mel_scale", "slaney"), a.get("norm", "slaney"),
           str(log_base), waveform.device)
    ex = _EXTRACTORS.get(key)
    if ex is None:
        ex = MelSpectrogram(target_sr, a["n_fft"], a["hop_length"], a["win_length"],
                            a["n_mels"], float(a["fmin"]), float(a["fmax"]),
                            a.get("mel_scale", "slaney"), a.get("norm", "slaney"),
                            1e-10, log_base, device=waveform.device)
        _EXTRACTORS[key] = ex
    log_mel = ex(waveform)[0]
    if print_shapes:
        # the reference prints the shape before the log; the fused kernel has the same shape
        print(f"[extract_mel] Mel spectrogram shape (before log): {log_mel.shape}")
        print(f"[extract_mel] Log-mel spectrogram shape: {log_mel.shape}")
        print(f"[extract_mel] Log-mel range: [{log_mel.min().item():.2f}, "
              f"{log_mel.max().item():.2f}]")
    return log_mel


def read_wav(path: Union[str, Path]) -> Tuple[torch.Tensor, int]:
    """(waveform [channels, time] float32, sample_rate) from a RIFF/WAVE file, normalised
    as torchaudio.load does: integer PCM divided by 2^(bits-1) (8-bit: (v - 128) / 128),
    IEEE float as stored.  Host-side file parsing (torchaudio is absent in this image)."""
    (tag, ch, sr, bits), pcm = riff_chunks(path)
    width = bits // 8
    n = len(pcm) // (width * ch)
    pcm = pcm[:n * width * ch]
    if tag == 3 and bits == 32:
        x = np.frombuffer(pcm, "<f4").astype(np.float32)
    elif tag == 3 and bits == 64:
        x = np.frombuffer(pcm, "<f8").astype(np.float32)
    elif tag == 1 and bits == 8:
        x = (np.frombuffer(pcm, np.uint8).astype(np.float32) - 128.0) / 128.0
    elif tag == 1 and bits == 16:
        x = np.frombuffer(pcm, "<i2").astype(np.float32) / 32768.0
    elif tag == 1 and bits == 24:
        b = np.frombuffer(pcm, np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        x = v.astype(np.float32) / float(1 << 23)
    elif tag == 1 and bits == 32:
        x = (np.frombuffer(pcm, "<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
    else:
        raise RuntimeError(f"{path}: unsupported WAV encoding (format {tag}, {bits} bits)")
    return torch.from_numpy(x.reshape(n, ch).T.copy()), sr


def extract_mel_from_file(audio_path: Union[str, Path], config: Optional[dict] = None,
                          config_path: str = "configs/config.yaml", device=None
                          ) -> Tuple[torch.Tensor, int]:
    """data/audio_processing.py:142-164: (log-mel [n_mels, T], sample_rate).  The file is
    parsed on the host (read_wav) and the waveform moved to the HIP device."""
    waveform, sample_rate = read_wav(audio_path)
    log_mel = extract_mel(waveform.to(default_device(device)), sample_rate, config, config_path)
    return log_mel, sample_rate


def save_mel(mel: torch.Tensor, output_path: Union[str, Path]) -> None:
    """data/audio_processing.py:167-184 (numpy .npy)."""
    output_path = Path(output_path)
    output_path.parent.mkdir(parents=True, exist_ok=True)
    np.save(output_path, mel.cpu().numpy())


def load_mel(mel_path: Union[str, Path]) -> torch.Tensor:
    """data/audio_processing.py:187-200."""
    return torch.from_numpy(np.load(mel_path)).float()
