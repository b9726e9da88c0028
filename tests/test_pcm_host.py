"""The release's PCM boundary on the CPU: the hfg_pcm_* C ABI (header, bindings, every
argument refusal: they come before any HIP call, so no device is needed), the two facts of
tests/pcm_oracle.py that keep the GPU tests from passing vacuously, the quantiser's
restatement on its edge values, and the WAV writer / reader."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from pcm_oracle import (SPECIALS, SPECIALS_NEAREST, SPECIALS_TRUNC, normalize_f32, normalize_ref,
                        pcm_signals, peak_ref, quantize_ref)

N, LENS = 8269, [8269, 3000, 385]
PCM_SYMBOLS = {"hfg_pcm_peak", "hfg_pcm_to_float", "hfg_pcm_offsets", "hfg_pcm_from_float"}


@pytest.fixture(scope="module")
def pcmmod(pkg):
    return importlib.import_module("tts_sambert_hifigan_amd.pcm")


def test_pcm_header_and_signatures_in_sync(pkg):
    """include/hifigan_hip_pcm.h declares exactly the four entries, each exported and bound,
    and hifigan_hip.h includes it."""
    lib = pkg.load_library()
    src = open(os.path.join(ROOT, "include", "hifigan_hip_pcm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    syms = set(re.findall(r"\b(hfg_[a-z0-9_]+)\s*\(", src))
    assert syms == PCM_SYMBOLS == set(pkg._lib.PCM_SIGNATURES)
    for s in syms:
        assert hasattr(lib, s), f"missing export {s}"
        assert getattr(lib, s).argtypes == pkg._lib.PCM_SIGNATURES[s][1]
    assert '#include "hifigan_hip_pcm.h"' in open(os.path.join(ROOT, "include",
                                                              "hifigan_hip.h")).read()
    for name, code in (("HFG_PCM_S16", 0), ("HFG_PCM_F32", 1), ("HFG_PCM_TRUNC", 0),
                       ("HFG_PCM_NEAREST", 1)):
        assert re.search(rf"\b{name}\s*=\s*{code}\b", src), name
    assert pkg._lib.PCM_DTYPES == {"int16": 0, "float32": 1}
    assert pkg._lib.PCM_ROUNDINGS == {"trunc": 0, "nearest": 1}
    assert pkg.pcm is importlib.import_module("tts_sambert_hifigan_amd.pcm")


def _refused(lib, rc):
    assert rc == -22
    assert lib.hfg_mel_last_error(), "no message"


def test_pcm_entries_refuse_bad_arguments(pkg):
    """Every HFG_EINVAL refusal, on host buffers and without a device: NULL data pointers, B
    outside [1, 65535], n_samples < 1, an unknown dtype or rounding code, a non-finite gain."""
    lib = pkg.load_library()
    buf = ctypes.cast((ctypes.c_float * 16)(), ctypes.c_void_p)
    inf, nan = float("inf"), float("nan")
    for B, n in [(0, 8), (-1, 8), (65536, 8), (1, 0), (1, -4)]:
        _refused(lib, lib.hfg_pcm_peak(buf, 0, B, n, None, buf, None))
        _refused(lib, lib.hfg_pcm_to_float(buf, 0, B, n, None, None, 0.95, buf, None))
        _refused(lib, lib.hfg_pcm_offsets(None, B, n, buf, None))
        _refused(lib, lib.hfg_pcm_from_float(buf, B, n, None, 0, None, buf, None))
    # NULL data pointers
    _refused(lib, lib.hfg_pcm_peak(None, 0, 1, 8, None, buf, None))
    _refused(lib, lib.hfg_pcm_peak(buf, 0, 1, 8, None, None, None))
    _refused(lib, lib.hfg_pcm_to_float(None, 0, 1, 8, None, None, 0.95, buf, None))
    _refused(lib, lib.hfg_pcm_to_float(buf, 0, 1, 8, None, None, 0.95, None, None))
    _refused(lib, lib.hfg_pcm_offsets(None, 1, 8, None, None))
    _refused(lib, lib.hfg_pcm_from_float(None, 1, 8, None, 0, None, buf, None))
    _refused(lib, lib.hfg_pcm_from_float(buf, 1, 8, None, 0, None, None, None))
    # codes
    for dtype in (-1, 2, 7):
        _refused(lib, lib.hfg_pcm_peak(buf, dtype, 1, 8, None, buf, None))
        assert b"dtype" in lib.hfg_mel_last_error()
        _refused(lib, lib.hfg_pcm_to_float(buf, dtype, 1, 8, None, None, 0.95, buf, None))
    for rounding in (-1, 2):
        _refused(lib, lib.hfg_pcm_from_float(buf, 1, 8, None, rounding, None, buf, None))
        assert b"rounding" in lib.hfg_mel_last_error()
    for gain in (inf, -inf, nan):
        _refused(lib, lib.hfg_pcm_to_float(buf, 0, 1, 8, None, buf, gain, buf, None))
        assert b"gain" in lib.hfg_mel_last_error()


def test_python_layer_refuses_cpu_tensors_and_bad_options(pcmmod):
    """No CPU fallback: a CPU tensor raises before the library is called."""
    pcm = torch.zeros(2, 16, dtype=torch.int16)
    with pytest.raises(RuntimeError, match="HIP tensor"):
        pcmmod.peak(pcm)
    with pytest.raises(RuntimeError, match="HIP tensor"):
        pcmmod.to_float(pcm)
    with pytest.raises(RuntimeError, match="HIP tensor"):
        pcmmod.to_pcm16(torch.zeros(2, 16))
    with pytest.raises(RuntimeError, match="rounding"):
        pcmmod.to_pcm16(torch.zeros(2, 16), rounding="floor")


def test_signal_peaks_and_the_length_that_changes_them():
    """Fact 1: the int16 batch does not clip, and item 2's peak over its first 385 samples
    differs from its row peak, so a kernel that reads past a length gives another answer."""
    s = pcm_signals(N)
    assert s.dtype == np.int16 and s.shape == (3, N)
    assert [int(np.abs(r.astype(np.int32)).max()) for r in s] == [16656, 10000, 12136]
    assert int(np.abs(s[2, :385].astype(np.int32)).max()) == 10446
    assert [float(peak_ref(s[b], n)) * 32768 for b, n in enumerate(LENS)][2] == 10446.0
    assert peak_ref(s[0], 0) == 0 and peak_ref(np.array([-32768], np.int16), 1) == 1.0


def test_float32_normalisation_is_not_the_releases(evidence):
    """Fact 2: evaluated in float32, the normalisation differs from the release's float64
    evaluation on more than 20 % of the samples of every item, so bitwise equality with
    normalize_ref tells the two apart."""
    s = pcm_signals(N)
    fracs = []
    for b, n in enumerate([N, N, N] + LENS):
        b %= 3
        a, r = normalize_f32(s[b], n), normalize_ref(s[b], n)
        assert a.dtype == r.dtype == np.float32 and a.shape == r.shape == (n,)
        fracs.append(float((a != r).mean()))
        assert np.abs(a.astype(np.float64) - r).max() <= 2.0 ** -23   # close, not equal
        assert np.abs(r).max() == np.float32(0.95)
    evidence("float32- vs float64-evaluated normalisation, share of samples that differ: "
             + ", ".join(f"{f:.1%}" for f in fracs))
    assert min(fracs[:3]) > 0.20


def test_normalize_ref_edges():
    """An all-zero item stays zero (divisor 1); a float32 item whose peak is subnormal is
    left undivided, one at the smallest normal number is divided."""
    assert not normalize_ref(np.zeros(7, np.int16), 7).any()
    assert normalize_ref(np.zeros(7, np.int16), 0).shape == (0,)
    tiny = np.finfo(np.float32).tiny
    sub = np.array([tiny / 2, -tiny / 4], np.float32)
    assert np.array_equal(normalize_ref(sub, 2, 1.0), sub)
    assert np.array_equal(normalize_ref(np.array([tiny, -tiny / 2], np.float32), 2, 1.0),
                          np.array([1.0, -0.5], np.float32))


def test_quantize_ref_edge_values():
    x = np.array([1, -1, 0.99999994, 0.5 / 32768, -0.5 / 32768, 1.5 / 32768, -1.5 / 32768,
                  np.nan, np.inf], np.float32)
    assert quantize_ref(x, "trunc").tolist() == [32767, -32768, 32767, 0, 0, 1, -1, 0, 32767]
    near = quantize_ref(x, "nearest").tolist()
    assert near[3:7] == [0, 0, 2, -2]
    assert near[:3] == [32767, -32768, 32767] and near[7:] == [0, 32767]
    assert np.array_equal(quantize_ref(SPECIALS, "trunc"), SPECIALS_TRUNC)
    assert np.array_equal(quantize_ref(SPECIALS, "nearest"), SPECIALS_NEAREST)
    # exact on the int16 grid, both modes
    grid = np.arange(-32768, 32768, dtype=np.int32)
    for mode in ("trunc", "nearest"):
        assert np.array_equal(quantize_ref((grid / 32768.0).astype(np.float32), mode),
                              grid.astype(np.int16))


@pytest.mark.parametrize("channels", [1, 2])
def test_wav_round_trip(pcmmod, pkg, tmp_path, channels):
    """write_wav -> read_wav_pcm16 is bitwise; the existing mel.read_wav of the same file is
    pcm / 32768 exactly; the header says PCM (tag 1), 16 bits."""
    melmod = importlib.import_module("tts_sambert_hifigan_amd.mel")
    s = torch.from_numpy(pcm_signals(1001)[:channels].copy())
    s[0, :4] = torch.tensor([-32768, 32767, 0, -1], dtype=torch.int16)
    path = tmp_path / "sub" / f"c{channels}.wav"
    pcmmod.write_wav(path, s[0] if channels == 1 else s, 22050)
    raw = path.read_bytes()
    assert raw[:4] == b"RIFF" and raw[8:16] == b"WAVEfmt "
    assert len(raw) == 44 + 2 * channels * 1001
    assert int.from_bytes(raw[4:8], "little") == len(raw) - 8
    assert int.from_bytes(raw[20:22], "little") == 1 and int.from_bytes(raw[34:36], "little") == 16
    assert int.from_bytes(raw[22:24], "little") == channels
    got, sr = pcmmod.read_wav_pcm16(path)
    assert sr == 22050 and got.dtype == torch.int16 and got.shape == (channels, 1001)
    assert torch.equal(got, s)
    f, sr2 = melmod.read_wav(path)
    assert sr2 == 22050 and f.dtype == torch.float32
    assert torch.equal(f, s.to(torch.float32) / 32768.0)


def test_read_wav_pcm16_refuses_other_encodings(pcmmod, tmp_path):
    import struct
    body = np.zeros(8, "<f4").tobytes()
    head = struct.pack("<4sI4s4sIHHIIHH4sI", b"RIFF", 36 + len(body), b"WAVE", b"fmt ", 16, 3, 1,
                       22050, 22050 * 4, 4, 32, b"data", len(body))
    p = tmp_path / "f32.wav"
    p.write_bytes(head + body)
    with pytest.raises(RuntimeError, match="unsupported"):
        pcmmod.read_wav_pcm16(p)
    (tmp_path / "junk.wav").write_bytes(b"not a wav file")
    with pytest.raises(RuntimeError, match="RIFF"):
        pcmmod.read_wav_pcm16(tmp_path / "junk.wav")
    with pytest.raises(RuntimeError):
        pcmmod.write_wav(tmp_path / "x.wav", torch.zeros(4), 22050)   # not int16
