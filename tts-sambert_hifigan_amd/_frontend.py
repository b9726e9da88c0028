"""What the audio front end's modules (``mel.py``, ``pcm.py``) share: the ``hfg_mel_last_error``
check, ctypes arguments from tensors, validated per-item lengths, handle ownership, the
RIFF/WAVE chunk walk."""
from __future__ import annotations

import ctypes
import struct
from ctypes import c_void_p
from pathlib import Path

import torch

from . import _lib
from .hifigan import _lengths_on


def check(lib, rc):
    if rc != 0:
        raise _lib.HfgError(rc, lib.hfg_mel_last_error().decode())


def stream(device) -> c_void_p:
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t) -> c_void_p:
    return c_void_p(t.data_ptr()) if t is not None else None


def float_ptr(t):
    """A host float32 tensor as ``const float*``."""
    return ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_float))


def default_device(device=None) -> torch.device:
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return torch.device(device)


def lengths(lengths, B: int, N: int, device):
    """None, or the lengths as a device int32 [B]; host values are validated."""
    if lengths is None:
        return None
    if not (isinstance(lengths, torch.Tensor) and lengths.is_cuda):
        host = torch.as_tensor(lengths)
        if host.shape != (B,):
            raise RuntimeError(f"lengths must have shape [{B}]")
        if host.is_floating_point() or any(int(n) < 0 or int(n) > N for n in host.tolist()):
            raise RuntimeError(f"every length must be an integer in [0, {N}], got "
                               f"{host.tolist()}")
    lens_t = _lengths_on(lengths, device)
    if lens_t.shape != (B,):
        raise RuntimeError(f"lengths must have shape [{B}]")
    return lens_t


def riff_chunks(path):
    """((format tag, channels, sample rate, bits), the data chunk's bytes) of a RIFF/WAVE file,
    parsed on the host."""
    data = Path(path).read_bytes()
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise RuntimeError(f"{path}: not a RIFF/WAVE file")
    pos, fmt, pcm = 12, None, None
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        body = data[pos + 8:pos + 8 + size]
        if cid == b"fmt ":
            tag, ch, sr, _, _, bits = struct.unpack("<HHIIHH", body[:16])
            if tag == 0xFFFE and len(body) >= 26:  # WAVE_FORMAT_EXTENSIBLE: subformat tag
                tag = struct.unpack("<H", body[24:26])[0]
            fmt = (tag, ch, sr, bits)
        elif cid == b"data":
            pcm = body
        pos += 8 + size + (size & 1)
    if fmt is None or pcm is None:
        raise RuntimeError(f"{path}: missing fmt or data chunk")
    return fmt, pcm


class HandleOwner:
    """Owns one front-end handle of the library: ``_open`` creates it on ``device`` (default:
    the current HIP device) and stores it as ``ptr``; it is destroyed with the object."""

    def _open(self, create: str, destroy: str, *args, device=None):
        self.lib = _lib.load_library()
        self.device = default_device(device)
        self._destroy = destroy
        h = c_void_p()
        check(self.lib, getattr(self.lib, create)(*args, self.device.index or 0, ctypes.byref(h)))
        self.ptr = h

    def __del__(self):
        try:
            if getattr(self, "ptr", None):
                getattr(self.lib, self._destroy)(self.ptr)
                self.ptr = None
        except Exception:
            pass
