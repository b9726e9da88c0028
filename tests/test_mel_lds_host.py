"""Host test: stating the DFT-GEMM pair's and resample_sinc's LDS sizes once (csrc/lds_layout.h)
moved no configuration between accepted and refused.

Before, hfg_mel_create admitted the pair by (31 hop + n_fft) * 4 * 33 / 32 <= 64 KiB (and 16
power rows of n_fft / 2 + 1 floats <= 64 KiB) while the launcher sized the skewed tile as
4 (span + span / hop + 1); hfg_resample_create and launch_resample both wrote out
(255 / phases + 1) stride + klen.  Those formulas are restated here and compared with what the
library answers now (hfg_debug_lds_bytes "stft_power_mfma", host-only creates).

CPU only: no device is touched.
"""
import ctypes
import math

import numpy as np
import pytest

KIB64 = 64 * 1024
CREATE_EDGE = 15887      # the largest span (31 hop + n_fft) the old create-time bound admits


def old_create_fits(n_fft, hop):
    return (((31 * hop + n_fft) * 4 * 33) // 32 <= KIB64) & (16 * (n_fft // 2 + 1) * 4 <= KIB64)


def old_launch_bytes(n_fft, hop):
    span = 31 * hop + n_fft
    return 4 * (span + span // hop + 1)


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


def test_old_bound_is_inside_the_launchers():
    """n_fft 2 .. 2048 (odd ones too) x hop 1 .. n_fft, the whole grid: every configuration the
    old create-time bound admits fits the launcher's tile, so taking the launcher's formula as
    the size refuses nothing that was accepted; the two differ (spans 15888 .. ~16350 fit the
    tile but were refused), which is why mel_dft_fits keeps the old bound as well."""
    n_fft = np.arange(2, 2049, dtype=np.int64)[:, None]
    hop = np.arange(1, 2049, dtype=np.int64)[None, :]
    grid = hop <= n_fft
    admitted = old_create_fits(n_fft, hop) & grid
    fits = (old_launch_bytes(n_fft, hop) <= KIB64) & (16 * (n_fft // 2 + 1) * 4 <= KIB64) & grid
    assert admitted.any() and (grid & ~admitted).any()
    assert not (admitted & ~fits).any()
    assert (fits & ~admitted).any()


def test_no_dft_configuration_changes_sides(lib):
    """Every n_fft 2 .. 2048 at the hops around both formulas' 64 KiB edges, the smallest hops,
    either side of the skew's 32, and hop = n_fft: admitted now exactly where it was, and the
    bytes are the launcher's."""
    arr = (ctypes.c_int * 2)()
    checked = admitted = 0
    for n_fft in range(2, 2049):
        edge = (CREATE_EDGE - n_fft) // 31
        edge2 = (KIB64 // 4 - n_fft) // 31
        hops = {1, 2, 3, 31, 32, 33, n_fft // 2, n_fft - 1, n_fft}
        hops |= set(range(edge - 3, edge + 4)) | set(range(edge2 - 3, edge2 + 4))
        for hop in sorted(h for h in hops if 1 <= h <= max(n_fft, edge2 + 3)):
            arr[0], arr[1] = n_fft, hop
            got = lib.hfg_debug_lds_bytes(b"stft_power_mfma", arr, 2)
            want = old_launch_bytes(n_fft, hop) if old_create_fits(n_fft, hop) else -1
            assert got == want, (n_fft, hop, got, want)
            assert got <= KIB64
            checked += 1
            admitted += got > 0
    assert admitted > 10000 and checked - admitted > 10000


@pytest.mark.parametrize("n_fft,forced", [(1000, False), (1024, True), (2046, False)])
def test_mel_create_edge(pkg, lib, n_fft, forced):
    """hfg_mel_create itself (host-only handles) at the old bound's edge, on an n_fft that is not
    a power of two and on one forced to the DFT path."""
    edge = (CREATE_EDGE - n_fft) // 31
    if forced:
        pkg.schedule_override("MEL_DFT", 1)
    try:
        for hop in (edge - 1, edge, edge + 1, edge + 2):
            c = pkg._lib.HfgMelConfig()
            c.sample_rate, c.n_fft, c.hop_length, c.win_length, c.n_mels = 22050, n_fft, hop, n_fft, 2
            c.f_min, c.f_max, c.log_eps, c.log_base = 0.0, 8000.0, 1e-10, 10
            h = ctypes.c_void_p()
            rc = lib.hfg_mel_create(ctypes.byref(c), -1, ctypes.byref(h))
            assert (rc == 0) == bool(old_create_fits(n_fft, hop)) == (hop <= edge), (hop, rc)
            if rc:
                assert rc == -22 and b"too large for the LDS frame tiles" in lib.hfg_mel_last_error()
            lib.hfg_mel_destroy(h)
    finally:
        pkg.schedule_clear("MEL_DFT")


def test_resample_create_edge(lib):
    """orig -> 1 Hz around the span's 64 KiB edge: accepted exactly where
    ((255 / phases + 1) stride + klen) floats fit, the formula both sides wrote out before."""
    seen = set()
    for orig in range(40, 80):
        width = math.ceil(6 * orig / np.float64(np.float32(0.99)))
        fits = 4 * (256 * orig + 2 * width + orig) <= KIB64
        h = ctypes.c_void_p()
        rc = lib.hfg_resample_create(orig, 1, 6, 0.99, -1, ctypes.byref(h))
        assert (rc == 0) == fits, (orig, rc)
        if rc:
            assert b"too large for the LDS input span" in lib.hfg_mel_last_error()
        lib.hfg_resample_destroy(h)
        seen.add(fits)
    assert seen == {True, False}
