"""The spectral distances on the CPU: the hfg_*_distance / hfg_stftdist_* C ABI on host-only
handles, metrics.SpectralDistance's arithmetic on hand-made sums, and the float64 oracle
(tests/spectral_distance_oracle.py) against the reference's recorded compute_stft_loss
(tests/golden/specdist_ref.json, written by tests/golden/make_specdist_golden.py)."""
import ctypes
import importlib
import json
import os
import re

import numpy as np
import pytest
import torch

import spectral_distance_oracle as O
from conftest import GOLDEN_DIR, ROOT
from release_mel_oracle import mel_f64

NEW_SYMBOLS = {"hfg_relmel_distance", "hfg_relmel_distance_workspace_bytes", "hfg_mel_distance",
               "hfg_mel_distance_workspace_bytes", "hfg_stftdist_create", "hfg_stftdist_destroy",
               "hfg_stftdist_set_window",
               "hfg_stftdist_frames", "hfg_stftdist_workspace_bytes", "hfg_stftdist_forward"}


@pytest.fixture(scope="module")
def metrics(pkg):
    return importlib.import_module("tts_sambert_hifigan_amd.metrics")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN_DIR, "specdist_ref.json")) as f:
        return json.load(f)


def test_header_and_signatures_in_sync(pkg):
    """Every entry point include/hifigan_hip_specdist.h declares is exported and bound with the
    signature of SPECDIST_SIGNATURES; the header reaches hifigan_hip.h by an #include line."""
    lib = pkg.load_library()
    src = open(os.path.join(ROOT, "include", "hifigan_hip_specdist.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    syms = set(re.findall(r"\b(hfg_[a-z0-9_]+)\s*\(", src))
    assert syms == NEW_SYMBOLS == set(pkg._lib.SPECDIST_SIGNATURES)
    assert not syms & set(pkg._lib.SIGNATURES)
    for s in syms:
        res, args = pkg._lib.SPECDIST_SIGNATURES[s]
        assert getattr(lib, s).restype == res and getattr(lib, s).argtypes == args, s
    assert '#include "hifigan_hip_specdist.h"' in open(os.path.join(ROOT, "include",
                                                                   "hifigan_hip.h")).read()


def _create(pkg, n_fft, hop, win, eps=0.0):
    lib = pkg.load_library()
    c = pkg._lib.HfgStftdistConfig(n_fft, hop, win, eps)
    h = ctypes.c_void_p()
    return lib, lib.hfg_stftdist_create(ctypes.byref(c), -1, ctypes.byref(h)), h


@pytest.mark.parametrize("cfg", [(1000, 120, 600), (8, 2, 8), (0, 1, 1), (1024, 0, 600),
                                 (1024, -3, 600), (1024, 120, 0), (1024, 120, 1025),
                                 (1024, 120, 600, -1e-5), (1024, 120, 600, float("nan")),
                                 (4096, 1024, 4096), (2048, 2000, 2048)])
def test_stftdist_create_refuses(pkg, cfg):
    """n_fft not a power of two or < 16, hop < 1, win outside [1, n_fft], eps <= 0 or NaN, and
    frame tiles beyond the LDS (n_fft 4096; n_fft 2048 with hop 2000: 128 KiB of FFT buffers
    plus two spans of 8048 floats): HFG_EINVAL with a message, no handle."""
    lib, rc, h = _create(pkg, *cfg)
    assert rc == -22 and not h.value
    assert lib.hfg_mel_last_error()
    assert lib.hfg_stftdist_create(None, -1, ctypes.byref(h)) == -22


def test_stftdist_reference_resolutions_host_only(pkg):
    for n_fft, hop, win in O.RESOLUTIONS + ((64, 24, 40), (16, 4, 16)):
        lib, rc, h = _create(pkg, n_fft, hop, win)
        assert rc == 0 and h.value, lib.hfg_mel_last_error()
        for n in (n_fft // 2 + 1, 1100, 3000, 8269):
            want = n // hop + 1 if n > n_fft // 2 else -1
            assert lib.hfg_stftdist_frames(h, n) == want, (n_fft, n)
        for n in (n_fft // 2, 1, 0, -7):
            assert lib.hfg_stftdist_frames(h, n) == -1
            assert lib.hfg_stftdist_workspace_bytes(h, 2, n) == 0
        # positive, and non-decreasing in B and in n
        grid = [[lib.hfg_stftdist_workspace_bytes(h, B, n) for n in (n_fft // 2 + 1, 3000, 8269, 262144)]
                for B in (1, 2, 3, 8)]
        assert all(v > 0 for row in grid for v in row)
        assert all(a <= b for row in grid for a, b in zip(row, row[1:]))
        assert all(a <= b for r0, r1 in zip(grid, grid[1:]) for a, b in zip(r0, r1))
        # one pair of doubles per block of 4 * frames-per-wave frames (2 up to n_fft 1024, else 1)
        fpb = 8 if n_fft <= 1024 else 4
        assert grid[1][2] == 2 * 16 * -(-(8269 // hop + 1) // fpb)
        w = torch.zeros(n_fft)
        w[(n_fft - win) // 2:(n_fft - win) // 2 + win] = torch.hann_window(win)
        assert lib.hfg_stftdist_set_window(h, ctypes.cast(w.data_ptr(), ctypes.POINTER(ctypes.c_float))) == 0
        assert lib.hfg_stftdist_set_window(h, None) == -22
        buf = (ctypes.c_double * 8)()
        p = ctypes.cast(buf, ctypes.c_void_p)
        assert lib.hfg_stftdist_forward(h, None, None, 1, 8269, None, None, 0, None, None, None) == -22
        assert lib.hfg_stftdist_forward(h, p, p, 1, 8269, None, p, 1 << 20, p, p, None) == -22
        assert b"host-only" in lib.hfg_mel_last_error()
        lib.hfg_stftdist_destroy(h)
    assert lib.hfg_stftdist_frames(None, 8269) == -1
    assert lib.hfg_stftdist_workspace_bytes(None, 1, 8269) == 0


def test_mel_handles_distance_host_only(pkg):
    """The distance entry points on host-only mel handles: workspace sizes, and refusals that
    launch nothing."""
    lib = pkg.load_library()
    rc_ = pkg._lib.HfgRelmelConfig(22050, 1024, 256, 1024, 80, 0.0, 8000.0, 0.0, 0.0)
    h = ctypes.c_void_p()
    assert lib.hfg_relmel_create(ctypes.byref(rc_), -1, ctypes.byref(h)) == 0
    assert lib.hfg_relmel_distance_workspace_bytes(h, 2, 8269) == 2 * 16 * 4     # 32 frames / 8
    assert lib.hfg_relmel_distance_workspace_bytes(h, 2, 384) == 0
    assert (lib.hfg_relmel_distance_workspace_bytes(h, 3, 8269)
            >= lib.hfg_relmel_distance_workspace_bytes(h, 2, 8269) > 0)
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.hfg_relmel_distance(h, None, 1, 8269, None, p, 32, p, 64, p, p, None) == -22
    assert lib.hfg_relmel_distance(h, p, 1, 8269, None, p, 32, p, 64, p, p, None) == -22
    assert b"host-only" in lib.hfg_mel_last_error()
    lib.hfg_relmel_destroy(h)
    c = pkg._lib.HfgMelConfig()
    c.sample_rate, c.n_fft, c.hop_length, c.win_length, c.n_mels = 22050, 1024, 256, 1024, 80
    c.f_min, c.f_max, c.mel_scale, c.norm, c.log_eps, c.log_base = 0.0, 8000.0, 0, 1, 1e-10, 10
    assert lib.hfg_mel_create(ctypes.byref(c), -1, ctypes.byref(h)) == 0
    assert lib.hfg_mel_distance_workspace_bytes(h, 2, 4173) == 2 * 16 * 3        # 17 frames / 8
    assert lib.hfg_mel_distance_workspace_bytes(h, 2, 512) == 0
    assert lib.hfg_mel_distance(h, p, 1, 8269, None, p, 33, p, 1 << 10, p, p, None) == -22
    assert b"host-only" in lib.hfg_mel_last_error()
    lib.hfg_mel_destroy(h)
    # n_fft 400: the DFT-GEMM path, refused with its reason before anything else
    c.n_fft, c.win_length, c.hop_length = 400, 400, 100
    assert lib.hfg_mel_create(ctypes.byref(c), -1, ctypes.byref(h)) == 0
    assert lib.hfg_mel_distance(h, p, 1, 8269, None, p, 33, p, 1 << 10, p, p, None) == -22
    assert b"DFT-GEMM" in lib.hfg_mel_last_error()
    lib.hfg_mel_destroy(h)


def test_spectral_distance_arithmetic(metrics):
    """per-item = sum / (rows max(frames, 1)); batch = sum of sums / (rows sum of frames)."""
    s1 = torch.tensor([80.0, 6.0, 0.0], dtype=torch.float64)
    s2 = torch.tensor([160.0, 3.0, 0.0], dtype=torch.float64)
    fr = torch.tensor([4, 1, 0], dtype=torch.int32)
    d = metrics.SpectralDistance(s1, s2, fr, rows=10)
    assert d.per_item_l1.tolist() == [2.0, 0.6, 0.0]
    assert d.per_item_l2.tolist() == [4.0, 0.3, 0.0]
    assert d.l1.item() == 86.0 / 50.0 and d.l2.item() == 163.0 / 50.0
    assert d.l1.dtype == torch.float64 and d.per_item_l1.dtype == torch.float64
    # not ragged: F.l1_loss / F.mse_loss of the underlying arrays
    g = torch.Generator().manual_seed(1)
    u, v = torch.randn(3, 10, 4, generator=g).double(), torch.randn(3, 10, 4, generator=g).double()
    e = metrics.SpectralDistance((u - v).abs().sum((1, 2)), ((u - v) ** 2).sum((1, 2)),
                                 torch.full((3,), 4, dtype=torch.int32), 10)
    assert abs(e.l1.item() - torch.nn.functional.l1_loss(u, v).item()) < 1e-15
    assert abs(e.l2.item() - torch.nn.functional.mse_loss(u, v).item()) < 1e-15
    # no frame anywhere: zeros, not NaN
    z = metrics.SpectralDistance(torch.zeros(2, dtype=torch.float64),
                                 torch.zeros(2, dtype=torch.float64),
                                 torch.zeros(2, dtype=torch.int32), 513)
    assert z.l1.item() == 0.0 and z.l2.item() == 0.0 and z.per_item_l2.tolist() == [0.0, 0.0]
    # the multi-resolution result: the mean over resolutions of each batch mean
    r = metrics.MultiResolutionSTFTResult([d, e])
    assert r.l1.item() == pytest.approx((d.l1.item() + e.l1.item()) / 2, abs=1e-15)
    assert r.l2.item() == pytest.approx((d.l2.item() + e.l2.item()) / 2, abs=1e-15)


def test_cpu_tensors_raise(metrics):
    a, _ = O.inputs(1100)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics._wav_rows(a, "mel_distance")
    with pytest.raises(TypeError):
        metrics.mel_distance(object(), a, a[:, None])
    assert metrics.REFERENCE_RESOLUTIONS == O.RESOLUTIONS


def test_oracle_against_the_reference(golden, evidence):
    """The float64 oracle against the reference's own float32 compute_stft_loss on the shared
    inputs.  The margin is 4 x the difference measured when the fixture was written (the
    reference's float32 FFT noise at quiet bins: up to 3.3e-5 on L1 ~ 2.08 and 6.0e-4 on
    L2 ~ 13.5)."""
    a, b = O.inputs()
    m1, m2 = golden["measured_max_diff"]["l1"], golden["measured_max_diff"]["l2"]
    assert 0 < m1 <= 3.4e-5 and 0 < m2 <= 6.1e-4
    l1s, l2s, worst1, worst2 = [], [], 0.0, 0.0
    for rec in golden["resolutions"]:
        r = (rec["n_fft"], rec["hop"], rec["win"])
        s1, s2, fr = O.stft_distance64(a, b, *r)
        assert fr.tolist() == [8269 // r[1] + 1] * 3
        _, _, l1, l2 = O.means(s1, s2, fr, r[0] // 2 + 1)
        l1s.append(l1)
        l2s.append(l2)
        worst1, worst2 = max(worst1, abs(l1 - rec["sc_loss"])), max(worst2, abs(l2 - rec["mag_loss"]))
        assert abs(l1 - rec["sc_loss"]) <= 4 * m1 and abs(l2 - rec["mag_loss"]) <= 4 * m2, r
    assert [tuple(r) for r in ((e["n_fft"], e["hop"], e["win"]) for e in golden["resolutions"])] \
        == list(O.RESOLUTIONS)
    o = golden["overall"]
    d1, d2 = abs(np.mean(l1s) - o["sc_loss"]), abs(np.mean(l2s) - o["mag_loss"])
    evidence(f"float64 STFT oracle vs the reference's float32 loss: L1 {max(worst1, d1):.2e} on "
             f"{o['sc_loss']:.4f}, L2 {max(worst2, d2):.2e} on {o['mag_loss']:.4f}")
    assert d1 <= 4 * m1 and d2 <= 4 * m2


def test_mel_oracle_sanity():
    """The CPU figures the GPU tests start from: per-item L1 of mel_f64(b) against mel_f64(a),
    unrounded.  0.1028 / 3.931 / 0.1478 are the three items at the ragged lengths the GPU
    tests use, [8269, 3000, 385] (item 0 over its full 8269 samples); over 8269 samples each
    the items give 0.1028 / 4.317 / 0.1099."""
    a, b = O.inputs()
    l1 = [np.abs(mel_f64(b[i:i + 1, :n]) - mel_f64(a[i:i + 1, :n])).mean()
          for i, n in enumerate([8269, 3000, 385])]
    assert np.allclose(l1, [0.1028, 3.931, 0.1478], rtol=2e-3), l1
    full = np.abs(mel_f64(b) - mel_f64(a)).mean(axis=(1, 2))
    assert np.allclose(full, [0.1028, 4.317, 0.1099], rtol=2e-3), full
