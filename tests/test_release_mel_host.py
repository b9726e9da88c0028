"""The release's mel front end on the CPU: the two restatements of tests/release_mel_oracle.py
against each other, the package's librosa filterbank against the oracle's and against the
torchaudio one, and the hfg_relmel_* C ABI on a host-only handle (device = -1)."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from release_mel_oracle import CONFIG, LOG_CLIP, librosa_mel, mel_f32, mel_f64, signals


@pytest.fixture(scope="module")
def melmod(pkg):
    return importlib.import_module("tts_sambert_hifigan_amd.mel")


def test_oracles_agree_as_far_as_float32_allows(evidence):
    """mel_f32 (the release's float32 torch ops) against mel_f64 (float64 spectrum) on
    signals(8269), 32 frames.  Measured with the CPU torch of the development machine:
    7.2e-6 where mel_f64 >= its max + ln(1e-3) (59 % of the entries), 2.8e-3 everywhere (the
    chirp's far bands near the 1e-5 floor, where the float32 FFT's own error dominates)."""
    wav = signals(8269)
    a, b = mel_f32(wav).numpy().astype(np.float64), mel_f64(wav)
    assert a.shape == b.shape == (2, 80, 32)
    strong = b >= b.max() + np.log(1e-3)
    err = np.abs(a - b)
    evidence(f"release mel oracles, f32 vs f64: strong ({strong.mean():.0%} of entries) "
             f"{err[strong].max():.2e}, all {err.max():.2e}")
    assert strong.mean() > 0.4
    assert err[strong].max() <= 2e-5
    assert err.max() <= 1e-2


def test_oracle_silence_is_the_clip():
    m = mel_f64(torch.zeros(1, 4096))
    assert m.shape == (1, 80, 16)
    assert (m == np.log(1e-5)).all()
    assert (mel_f32(torch.zeros(1, 4096)).numpy() == LOG_CLIP).all()


@pytest.mark.parametrize("sr,n_fft,n_mels,fmin,fmax", [(22050, 1024, 80, 0.0, 8000.0),
                                                       (22050, 1024, 80, 0.0, None),
                                                       (16000, 512, 40, 55.0, 7600.0),
                                                       (44100, 2048, 128, 0.0, 16000.0)])
def test_librosa_filterbank_matches_oracle(melmod, sr, n_fft, n_mels, fmin, fmax):
    """mel.librosa_mel_fn within one float32 ulp of the oracle's table, entry by entry."""
    got = melmod.librosa_mel_fn(sr, n_fft, n_mels, fmin, fmax)
    ref = librosa_mel(sr, n_fft, n_mels, fmin, fmax)
    assert got.dtype == np.float32 and got.shape == ref.shape == (n_mels, n_fft // 2 + 1)
    assert ((got != 0) == (ref != 0)).all()
    assert (np.abs(got - ref) <= np.spacing(np.abs(ref))).all()
    # every band has weight, and Slaney's area norm: the triangles' areas in Hz are ~1
    assert (got.sum(1) > 0).all()


def test_librosa_filterbank_is_not_torchaudios(melmod, evidence):
    """Close to the torchaudio table MelSpectrogram uses (<= 1e-7), but not the same table."""
    got = melmod.librosa_mel_fn(22050, 1024, 80, 0.0, 8000.0)
    ta = melmod.melscale_fbanks(513, 0.0, 8000.0, 80, 22050, "slaney", "slaney").numpy().T
    d = np.abs(got - ta).max()
    evidence(f"librosa vs torchaudio filterbank (22.05 kHz / 1024 / 80 / 0-8000): max diff {d:.2e}")
    assert d <= 1e-7
    assert not np.array_equal(got, ta)


def _cfg(pkg, **kw):
    c = pkg._lib.HfgRelmelConfig()
    v = dict(CONFIG, **kw)
    c.sampling_rate, c.n_fft, c.hop_size, c.win_size, c.num_mels = (
        v["sampling_rate"], v["n_fft"], v["hop_size"], v["win_size"], v["num_mels"])
    c.fmin, c.fmax = v["fmin"], v["fmax"]
    return c


def test_relmel_header_and_signatures_in_sync(pkg):
    """Every entry point include/hifigan_hip_relmel.h declares is exported and bound."""
    lib = pkg.load_library()
    src = open(os.path.join(ROOT, "include", "hifigan_hip_relmel.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    syms = set(re.findall(r"\b(hfg_[a-z0-9_]+)\s*\(", src))
    assert syms == set(pkg._lib.RELMEL_SIGNATURES) and len(syms) == 5
    for s in syms:
        assert hasattr(lib, s), f"missing export {s}"
    assert '#include "hifigan_hip_relmel.h"' in open(os.path.join(ROOT, "include",
                                                                 "hifigan_hip.h")).read()


def test_relmel_handle_host_only(pkg):
    lib = pkg.load_library()
    h = ctypes.c_void_p()
    assert lib.hfg_relmel_create(ctypes.byref(_cfg(pkg)), -1, ctypes.byref(h)) == 0
    for n, frames in [(385, 1), (513, 2), (8269, 32), (384, -1), (0, -1), (-5, -1)]:
        assert lib.hfg_relmel_frames(h, n) == frames, n
    assert lib.hfg_relmel_forward(h, None, 1, 8269, None, None, None, None) == -22
    # non-NULL pointers: refused because the handle is host-only, nothing is launched
    buf = (ctypes.c_float * 4)()
    assert lib.hfg_relmel_forward(h, buf, 1, 8269, None, buf, None, None) == -22
    assert b"host-only" in lib.hfg_mel_last_error()
    w = torch.hann_window(1024)
    fb = torch.from_numpy(np.ascontiguousarray(librosa_mel(22050, 1024, 80, 0.0, 8000.0).T))
    fp = ctypes.POINTER(ctypes.c_float)
    assert lib.hfg_relmel_set_tables(h, ctypes.cast(w.data_ptr(), fp),
                                     ctypes.cast(fb.data_ptr(), fp)) == 0
    assert lib.hfg_relmel_set_tables(h, None, None) == -22
    lib.hfg_relmel_destroy(h)
    # n_fft 64, hop 60: the pad p = 2 is not the limit, n >= hop is
    assert lib.hfg_relmel_create(ctypes.byref(_cfg(pkg, n_fft=64, hop_size=60, win_size=64)), -1,
                                 ctypes.byref(h)) == 0
    assert lib.hfg_relmel_frames(h, 59) == -1 and lib.hfg_relmel_frames(h, 60) == 1
    lib.hfg_relmel_destroy(h)


@pytest.mark.parametrize("kw", [dict(n_fft=1000, win_size=1000), dict(hop_size=255),
                                dict(win_size=2048), dict(fmax=0.5, fmin=1.0),
                                dict(fmax=8000.0, fmin=8000.0), dict(n_fft=8, hop_size=2, win_size=8),
                                dict(n_fft=4096, hop_size=1024, win_size=4096)])
def test_relmel_create_refuses(pkg, kw):
    """n_fft not a power of two, an odd n_fft - hop, win_size > n_fft, fmax <= fmin with
    fmax > 0, n_fft < 16, and an n_fft whose frame tile does not fit the LDS: HFG_EINVAL (-22)
    with a message, no handle."""
    lib = pkg.load_library()
    h = ctypes.c_void_p()
    assert lib.hfg_relmel_create(ctypes.byref(_cfg(pkg, **kw)), -1, ctypes.byref(h)) == -22
    assert not h.value
    assert lib.hfg_mel_last_error()


def test_relmel_fmax_null_is_nyquist(pkg):
    lib = pkg.load_library()
    h = ctypes.c_void_p()
    for fmax in (0.0, -1.0):
        assert lib.hfg_relmel_create(ctypes.byref(_cfg(pkg, fmax=fmax)), -1, ctypes.byref(h)) == 0
        lib.hfg_relmel_destroy(h)


def test_existing_mel_handle_unchanged(pkg):
    """The hfg_mel_* handle answers as before next to the new section."""
    lib = pkg.load_library()
    c = pkg._lib.HfgMelConfig()
    c.sample_rate, c.n_fft, c.hop_length, c.win_length, c.n_mels = 22050, 1024, 256, 1024, 80
    c.f_min, c.f_max, c.mel_scale, c.norm, c.log_eps, c.log_base = 0.0, 8000.0, 0, 1, 1e-10, 10
    h = ctypes.c_void_p()
    assert lib.hfg_mel_create(ctypes.byref(c), -1, ctypes.byref(h)) == 0
    assert lib.hfg_mel_frames(h, 8269) == 8269 // 256 + 1
    assert lib.hfg_mel_workspace_bytes(h, 2, 8269) == 256
    assert lib.hfg_mel_forward(h, None, 1, 8269, None, None, 0, None) == -22
    lib.hfg_mel_destroy(h)
