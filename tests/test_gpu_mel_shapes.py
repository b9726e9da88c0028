"""The reference mel front end on the device off its one shape (mel_cases.py): logmel_fft at
win_length < n_fft, hops that do not divide n_fft or reach it, 13 .. 128 bands, empty bands, htk /
norm=None, f_min > 0, n_fft 16 .. 2048 and every frame-count residue of its block;
stft_power_mfma + mel_log at the n_fft it exists for (400, 1200, 126, 50) and forced at 1024,
over the block tails of both kernels.

Truth: oracle.mel_torch.log_mel64 (float64 spectrum).  Bars, none new: FFT path 1e-5 (log10) on
every band, empty ones included; DFT path 1e-4 on bands within 2 decades of the item's maximum
and 5e-4 on the rest (all within 6 decades: test_mel_shapes_host.py).  Beyond the bars: every
item of the 3-item batch is bitwise its solo run, nothing outside the arguments is touched, the
unforced DFT cases are shown to take the DFT path by their workspace size, and refusals raise
before anything is launched."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import mel_cases as MC

pytestmark = pytest.mark.gpu

ALL_DFT = MC.DFT_CONFIGS + [MC.DFT_FORCED]
GUARD = 4096   # floats either side of every argument of the guard test


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def melmod(pkg):
    return importlib.import_module("tts_sambert_hifigan_amd.mel")


def _ids(cfgs):
    return [c["name"] for c in cfgs]


def _extractor(melmod, cfg, dev, sched):
    if cfg is MC.DFT_FORCED:
        sched("MEL_DFT", 1)     # read when the handle is created
    return melmod.MelSpectrogram(**MC.class_kwargs(cfg), device=dev)


def _workspace(ext, B, n):
    return int(ext.lib.hfg_mel_workspace_bytes(ext.ptr, B, n))


def _assert_path(ext, cfg, B, n):
    """The workspace size tells the path: 256 bytes for logmel_fft, the power spectra
    [B][frames][n_bins] fp32 for stft_power_mfma + mel_log."""
    want = 256 if cfg in MC.FFT_CONFIGS else MC.dft_workspace_bytes(cfg, B, n)
    assert _workspace(ext, B, n) == want, (cfg["name"], n)


def _run_lengths(ext, cfg, dev):
    """{n: device output [3, n_mels, frames] on the CPU} with shape, path and batch independence
    asserted: every item of the batch is bitwise its own B = 1 run."""
    out = {}
    for n in MC.lengths(cfg):
        wav, ref = MC.mel_ref(cfg["name"], n)
        _assert_path(ext, cfg, 3, n)
        got = ext(wav.to(dev)).cpu()
        assert got.shape == ref.shape == (3, cfg["n_mels"], n // cfg["hop_length"] + 1), (cfg["name"], n)
        assert bool(torch.isfinite(got).all()), (cfg["name"], n)
        for b in range(3):
            solo = ext(wav[b:b + 1].to(dev)).cpu()
            assert torch.equal(solo[0], got[b]), (cfg["name"], n, b)
        out[n] = got
    return out


@pytest.mark.parametrize("cfg", MC.FFT_CONFIGS, ids=_ids(MC.FFT_CONFIGS))
def test_fft_path_shapes(pkg, dev, melmod, sched, evidence, cfg):
    """logmel_fft: every band of every item within 1e-5 (log10) of log_mel64 at every length of
    the configuration; one handle serves all of its lengths."""
    ext = _extractor(melmod, cfg, dev, sched)
    worst, at = 0.0, None
    got = _run_lengths(ext, cfg, dev)
    for n, g in got.items():
        e = float((g.double() - MC.mel_ref(cfg["name"], n)[1]).abs().max())
        if e > worst:
            worst, at = e, n
    evidence(f"mel fft {cfg['name']}: {len(got)} lengths x 3 items, worst |log10 mel - fp64 oracle| "
             f"{worst:.2e} at N = {at} (bar {MC.FFT_BAR:g})")
    assert worst <= MC.FFT_BAR, (worst, at)
    if cfg["name"] in MC.EMPTY_BANDS:    # a band with no bin is log10(eps) in every frame
        g = got[MC.lengths(cfg)[-1]]
        flat = (g == g[:, :, :1]).all(-1).all(0) & (g[0, :, 0] < -9.99)
        assert int(flat.sum()) == MC.EMPTY_BANDS[cfg["name"]]


@pytest.mark.parametrize("cfg", ALL_DFT, ids=_ids(ALL_DFT))
def test_dft_path_shapes(pkg, dev, melmod, sched, evidence, cfg):
    """stft_power_mfma + mel_log, unforced where n_fft is not a power of two: 1e-4 on the bands
    within 2 decades of the item's maximum, 5e-4 on all (every band is within 6 decades), against
    log_mel64."""
    ext = _extractor(melmod, cfg, dev, sched)
    ws, wa, at = 0.0, 0.0, None
    got = _run_lengths(ext, cfg, dev)
    for n, g in got.items():
        ref = MC.mel_ref(cfg["name"], n)[1]
        e = (g.double() - ref).abs()
        for b in range(3):
            strong, big = MC.dft_masks(ref[b])
            assert bool(big.all())
            ws = max(ws, float(e[b][strong].max()))
            if float(e[b].max()) > wa:
                wa, at = float(e[b].max()), n
    evidence(f"mel dft {cfg['name']}: {len(got)} lengths x 3 items, worst |log10 mel - fp64 oracle| "
             f"strong bands {ws:.2e} (bar {MC.DFT_BAR_STRONG:g}), all bands {wa:.2e} at N = {at} "
             f"(bar {MC.DFT_BAR:g}); workspace = 4 B frames n_bins: the DFT path")
    assert ws <= MC.DFT_BAR_STRONG, ws
    assert wa <= MC.DFT_BAR, (wa, at)


def _guarded(n_floats, fill, dev):
    """(buffer, view): a view of n_floats floats with GUARD floats of `fill` either side."""
    buf = torch.full((n_floats + 2 * GUARD,), fill, dtype=torch.float32, device=dev)
    return buf, buf[GUARD:GUARD + n_floats]


def _guards_intact(buf, n_floats, fill):
    g = torch.cat([buf[:GUARD], buf[GUARD + n_floats:]]).cpu()
    return bool(torch.isnan(g).all()) if fill != fill else bool((g == fill).all())


@pytest.mark.parametrize("cfg", MC.FFT_CONFIGS + ALL_DFT, ids=_ids(MC.FFT_CONFIGS + ALL_DFT))
def test_no_access_outside_the_arguments(pkg, dev, melmod, sched, cfg):
    """hfg_mel_forward on slices of larger device tensors: the wav lies between 1e30 guards, the
    mel (and on the DFT path the workspace) is pre-filled with NaN between NaN guards.  The mel
    comes back without a NaN and bitwise the plain call's, and no guard has moved: a read past
    either end of an item would put 1e30 (or NaN) into a band, a write past the output would
    show in its guard.  At the shortest length and at one block tail."""
    ext = _extractor(melmod, cfg, dev, sched)
    lib = pkg.load_library()
    nan = float("nan")
    for n in MC.guard_lengths(cfg):
        wav = MC.mel_ref(cfg["name"], n)[0]
        plain = ext(wav.to(dev))
        T = n // cfg["hop_length"] + 1
        wbuf, w = _guarded(3 * n, 1e30, dev)
        w.copy_(wav.to(dev).reshape(-1))
        mbuf, m = _guarded(3 * cfg["n_mels"] * T, nan, dev)
        ws_bytes = _workspace(ext, 3, n)
        assert ws_bytes % 4 == 0
        sbuf, s = _guarded(ws_bytes // 4, nan, dev)
        rc = lib.hfg_mel_forward(ext.ptr, ctypes.c_void_p(w.data_ptr()), 3, n,
                                 ctypes.c_void_p(m.data_ptr()), ctypes.c_void_p(s.data_ptr()),
                                 ws_bytes, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        assert rc == 0, lib.hfg_mel_last_error()
        torch.cuda.synchronize()
        assert not bool(torch.isnan(m).any()), (cfg["name"], n)
        assert torch.equal(m.reshape(plain.shape), plain), (cfg["name"], n)
        assert _guards_intact(wbuf, 3 * n, 1e30) and torch.equal(w, wav.to(dev).reshape(-1))
        assert _guards_intact(mbuf, m.numel(), nan), (cfg["name"], n)
        assert _guards_intact(sbuf, s.numel(), nan), (cfg["name"], n)
        if cfg not in MC.FFT_CONFIGS:     # every power spectrum was written, none is NaN
            assert not bool(torch.isnan(s).any()), (cfg["name"], n)


def test_refusals_launch_nothing(pkg, dev, melmod):
    """N = n_fft / 2 (the reflect pad needs one sample more), odd n_fft, win_length > n_fft and a
    non-power-of-two n_fft too large for the DFT tiles raise from the Python class; the refused
    call writes nothing to its output."""
    HfgError = pkg._lib.HfgError
    for c in MC.REFUSED_CONFIGS:
        with pytest.raises(HfgError):
            melmod.MelSpectrogram(**MC.class_kwargs(c), device=dev)
    lib = pkg.load_library()
    for cfg in (MC.FFT_CONFIGS[1], MC.DFT_CONFIGS[0]):
        ext = melmod.MelSpectrogram(**MC.class_kwargs(cfg), device=dev)
        n = cfg["n_fft"] // 2
        wav = torch.zeros(3, n, device=dev)
        with pytest.raises(HfgError, match="reflect padding"):
            ext(wav)
        T = n // cfg["hop_length"] + 1
        mel = torch.full((3, cfg["n_mels"], T), float("nan"), device=dev)
        ws = torch.zeros(max(_workspace(ext, 3, n), 4), dtype=torch.uint8, device=dev)
        rc = lib.hfg_mel_forward(ext.ptr, ctypes.c_void_p(wav.data_ptr()), 3, n,
                                 ctypes.c_void_p(mel.data_ptr()), ctypes.c_void_p(ws.data_ptr()),
                                 ws.numel(), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize()
        assert rc == -22 and bool(torch.isnan(mel).all())


def test_extract_mel_off_default(pkg, dev, melmod):
    """extract_mel at 1024 / 200 / 800 on a stereo 16 kHz wave: resampled per channel, the mono
    mean, then the mel — against R.resample then the oracle, under the propagated tolerance of
    test_extract_mel_resamples_and_prints (_check against the oracle of the oracle-resampled
    wave)."""
    from oracle import mel_torch as M, resample_np as R
    from test_gpu_mel import _check, _signals   # the existing bars and chirp, unchanged
    c = MC.EXTRACT_CONFIG
    cfg = {"audio": {"sample_rate": c["sample_rate"], "n_fft": c["n_fft"], "hop_length": c["hop_length"],
                     "win_length": c["win_length"], "n_mels": c["n_mels"], "fmin": 0, "fmax": 8000,
                     "log_base": 10.0}}
    stereo = _signals(16000)
    mel = melmod.extract_mel(stereo.to(dev), sample_rate=16000, config=cfg)
    ref_wav = torch.from_numpy(R.resample(stereo.numpy(), 16000, 22050)).mean(0)
    assert mel.shape == (80, 22050 // 200 + 1)
    _check(mel.cpu(), M.log_mel(ref_wav, c))
