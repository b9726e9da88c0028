"""The public HiFi-GAN release's PCM boundary on the HIP device (``include/hifigan_hip_pcm.h``).

The release reads 16-bit PCM, divides by ``MAX_WAV_VALUE`` and peak-normalises with
``normalize(audio) * 0.95`` (``meldataset.py``); ``inference.py`` multiplies the Generator's
output by ``MAX_WAV_VALUE`` and casts to int16.  Here both ends are kernels of
``libhifigan_hip.so`` (``csrc/pcm.hip``), ragged like the rest of the chain:

* :func:`peak` — per-item ``max |x|`` as a device float32 ``[B]``, no sync: also the
  release's ``|wav| > 1`` check;
* :func:`to_float` — int16 / float32 ``[B, N]`` → float32 ``[B, N]``, optionally the release's
  float64-evaluated peak normalisation, bitwise;
* :func:`to_pcm16` — float32 → int16 with saturation (``+1.0`` is 32767, not the release's
  wrapped −32768), padded ``[B, L]`` or packed ``(flat, offsets)``;
* :func:`read_wav_pcm16` / :func:`write_wav` — 16-bit RIFF/WAVE files on the host.

``lengths`` is a sequence of ints or an int tensor ``[B]``.  Host lengths are validated
(shape ``[B]``, each in ``[0, N]``); a device tensor is never read back (the kernels clamp it
into ``[0, N]``).  There is no CPU fallback: a CPU tensor raises.
"""
from __future__ import annotations

import math
import struct
from pathlib import Path
from typing import Tuple, Union

import numpy as np
import torch

from . import _lib
from ._frontend import (check as _check, lengths as _lengths, ptr as _ptr, riff_chunks,
                        stream as _stream)


def _dtype_code(wav) -> int:
    return _lib.PCM_DTYPES["int16" if wav.dtype == torch.int16 else "float32"]


def _rows(wav: torch.Tensor, who: str, dtypes) -> torch.Tensor:
    if not (isinstance(wav, torch.Tensor) and wav.is_cuda):
        raise RuntimeError(f"pcm.{who} (MI355X) needs a HIP tensor; no CPU fallback")
    if wav.dim() != 2 or wav.shape[0] < 1 or wav.shape[1] < 1:
        raise RuntimeError(f"pcm.{who}: expected wav [B, N] with B, N >= 1, got "
                           f"{tuple(wav.shape)}")
    if wav.dtype not in dtypes:
        raise RuntimeError(f"pcm.{who}: expected {' or '.join(str(d) for d in dtypes)}, got "
                           f"{wav.dtype}")
    return wav.detach().contiguous()


def _peak(lib, wav, lens_t) -> torch.Tensor:
    B, N = wav.shape
    out = torch.empty(B, device=wav.device, dtype=torch.float32)
    with torch.cuda.device(wav.device):
        _check(lib, lib.hfg_pcm_peak(_ptr(wav), _dtype_code(wav), B, N,
                                     _ptr(lens_t), _ptr(out), _stream(wav.device)))
    return out


def peak(wav: torch.Tensor, lengths=None) -> torch.Tensor:
    """wav [B, N] int16 or float32 on the HIP device → ``max |x|`` over each item's length,
    float32 [B] on the device (int16: ``|s| / 32768``, so −32768 gives exactly 1.0).  A NaN
    inside an item's length makes that item's peak NaN; an empty item's peak is 0."""
    wav = _rows(wav, "peak", (torch.int16, torch.float32))
    return _peak(_lib.load_library(), wav, _lengths(lengths, *wav.shape, wav.device))


def to_float(wav: torch.Tensor, lengths=None, normalize: bool = False, gain: float = 0.95
             ) -> torch.Tensor:
    """wav [B, N] int16 or float32 on the HIP device → float32 [B, N], 0 past each length.
    Plain: ``s / 32768`` (``read_wav``'s value; float32 is passed through).  ``normalize``:
    the release's ``normalize(audio / 32768.0) * gain``, a float64 division by the item's peak
    and a float64 product rounded once, bitwise what numpy gives; an item whose peak is below
    the smallest normal number (for int16: all zeros) is left undivided."""
    wav = _rows(wav, "to_float", (torch.int16, torch.float32))
    if not math.isfinite(float(gain)):
        raise RuntimeError(f"pcm.to_float: gain must be finite, got {gain!r}")
    lib = _lib.load_library()
    B, N = wav.shape
    lens_t = _lengths(lengths, B, N, wav.device)
    pk = _peak(lib, wav, lens_t) if normalize else None
    out = torch.empty(B, N, device=wav.device, dtype=torch.float32)
    with torch.cuda.device(wav.device):
        _check(lib, lib.hfg_pcm_to_float(_ptr(wav), _dtype_code(wav), B, N,
                                         _ptr(lens_t), _ptr(pk), float(gain), _ptr(out),
                                         _stream(wav.device)))
    return out


def to_pcm16(wav: torch.Tensor, lengths=None, rounding: str = "trunc", packed: bool = False):
    """wav [B, L] or [B, 1, L] float32 on the HIP device → int16:
    ``sat16(round(x * 32768))``, ``rounding`` "trunc" (toward zero, the release's
    ``astype('int16')``) or "nearest" (to nearest even); ±1.0 and beyond saturate to
    32767 / −32768, NaN gives 0.  Padded: int16 [B, L], 0 past each length.  ``packed``:
    ``(flat int16, offsets int64 [B + 1])`` with item b at ``flat[offsets[b]:offsets[b + 1]]``;
    flat holds ``sum(lengths)`` samples for host lengths and ``B * L`` for a device tensor
    (whose sum is not read back; the part past ``offsets[B]`` is not written)."""
    if rounding not in _lib.PCM_ROUNDINGS:
        raise RuntimeError(f"pcm.to_pcm16: rounding must be one of "
                           f"{sorted(_lib.PCM_ROUNDINGS)}, got {rounding!r}")
    if isinstance(wav, torch.Tensor) and wav.dim() == 3 and wav.shape[1] == 1:
        wav = wav[:, 0]
    wav = _rows(wav, "to_pcm16", (torch.float32,))
    lib = _lib.load_library()
    B, L = wav.shape
    lens_t = _lengths(lengths, B, L, wav.device)
    dev, st = wav.device, _stream(wav.device)
    code = _lib.PCM_ROUNDINGS[rounding]
    with torch.cuda.device(dev):
        if not packed:
            out = torch.empty(B, L, device=dev, dtype=torch.int16)
            _check(lib, lib.hfg_pcm_from_float(_ptr(wav), B, L, _ptr(lens_t), code, None,
                                               _ptr(out), st))
            return out
        if lengths is None or (isinstance(lengths, torch.Tensor) and lengths.is_cuda):
            total = B * L
        else:
            total = sum(int(n) for n in torch.as_tensor(lengths).tolist())
        offsets = torch.empty(B + 1, device=dev, dtype=torch.int64)
        _check(lib, lib.hfg_pcm_offsets(_ptr(lens_t), B, L, _ptr(offsets), st))
        # at least one element, so an all-empty batch still hands the kernel a pointer
        flat = torch.empty(max(total, 1), device=dev, dtype=torch.int16)
        _check(lib, lib.hfg_pcm_from_float(_ptr(wav), B, L, _ptr(lens_t), code, _ptr(offsets),
                                           _ptr(flat), st))
        return flat[:total], offsets


def read_wav_pcm16(path: Union[str, Path]) -> Tuple[torch.Tensor, int]:
    """(int16 [channels, time], sample_rate) from a 16-bit PCM RIFF/WAVE file, the samples as
    stored (``mel.read_wav`` returns them divided by 32768).  Any other encoding raises."""
    (tag, ch, sr, bits), pcm = riff_chunks(path)
    if tag != 1 or bits != 16 or ch < 1:
        raise RuntimeError(f"{path}: unsupported WAV encoding (format {tag}, {bits} bits); "
                           "read_wav_pcm16 takes 16-bit PCM only")
    n = len(pcm) // (2 * ch)
    x = np.frombuffer(pcm[:n * 2 * ch], "<i2").astype(np.int16)
    return torch.from_numpy(x.reshape(n, ch).T.copy()), sr


def write_wav(path: Union[str, Path], pcm: torch.Tensor, sample_rate: int) -> None:
    """Write int16 [time] or [channels, time] (any device) as a RIFF/WAVE file: format tag 1
    (PCM), 16 bits, channels interleaved."""
    if not isinstance(pcm, torch.Tensor) or pcm.dtype != torch.int16 or pcm.dim() not in (1, 2):
        raise RuntimeError("write_wav: expected an int16 tensor [time] or [channels, time]")
    if pcm.dim() == 1:
        pcm = pcm[None]
    ch, n = pcm.shape
    sr = int(sample_rate)
    if not (1 <= ch <= 65535) or not (1 <= sr < 2 ** 32) or 2 * ch * n >= 2 ** 32 - 36:
        raise RuntimeError(f"write_wav: cannot store [{ch}, {n}] at {sample_rate} Hz in a "
                           "RIFF/WAVE file")
    body = pcm.detach().cpu().numpy().T.astype("<i2").tobytes()
    head = struct.pack("<4sI4s4sIHHIIHH4sI", b"RIFF", 36 + len(body), b"WAVE",
                       b"fmt ", 16, 1, ch, sr, sr * ch * 2, ch * 2, 16, b"data", len(body))
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_bytes(head + body)
