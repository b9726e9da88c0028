"""resample_sinc off its one length (mel_cases.py): nine rate pairs — two phases (11025 -> 22050),
the long filters of 32 kHz and 96 kHz sources (klen 658 / 694), down- and upsampling by 160 and
the smallest ratios 2 -> 3 / 3 -> 2 — each at inputs shorter than the filter half-width, around
one stride, and at outputs ending on or next to the kernel's 256-output block edges.

Truth: oracle.resample_np.resample (float64 accumulation).  Bars, none new: 2e-6 x max|x| on
the output, 1e-7 on the kernel table.  Beyond the bar: every row of the 3-row batch is bitwise
its solo run; unit impulses at the first, middle and last sample return the filter's own taps
(a phase or offset slip of one changes them in the first digit); nothing outside the arguments
is touched."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import mel_cases as MC
from oracle import resample_np as R

pytestmark = pytest.mark.gpu

PAIRS = list(MC.RESAMPLE_PAIRS)
PAIR_IDS = [f"{o}-{n}" for o, n in PAIRS]
GUARD = 4096


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def melmod(pkg):
    return importlib.import_module("tts_sambert_hifigan_amd.mel")


@pytest.mark.parametrize("orig,new", PAIRS, ids=PAIR_IDS)
def test_resample_shapes(pkg, dev, melmod, evidence, orig, new):
    rs = melmod.Resample(orig, new, device=dev)
    k, width = rs.kernel()
    rk, rw = R.sinc_kernel(orig, new)
    assert width == rw and k.shape == rk.shape
    assert np.abs(k.numpy() - rk).max() <= MC.KERNEL_BAR
    worst, worst_imp, at = 0.0, 0.0, None
    lens = MC.resample_lengths(orig, new)
    # the block-edge output lengths this pair can produce are all among the cases
    assert {rs.out_len(n) for n in lens} & set(MC.OUT_TARGETS) == set(MC.OUT_HIT[(orig, new)])
    for n in lens:
        x = MC.resample_rows(n, orig)
        ref = R.resample(x, orig, new)
        xd = torch.from_numpy(np.array(x)).to(dev)
        y = rs(xd).cpu().numpy()
        assert y.shape == ref.shape == (3, MC.out_len(orig, new, n)), n
        scale = float(np.abs(x).max())
        err = float(np.abs(y - ref).max()) / scale
        if err > worst:
            worst, at = err, n
        for b in range(3):
            solo = rs(xd[b:b + 1]).cpu().numpy()
            assert np.array_equal(solo[0], y[b]), (n, b)
        imp = MC.impulses(n)
        yi = rs(torch.from_numpy(imp).to(dev)).cpu().numpy()
        ri = R.resample(imp, orig, new)
        assert yi.shape == ri.shape
        worst_imp = max(worst_imp, float(np.abs(yi - ri).max()))
    evidence(f"resample {orig}->{new}: {len(lens)} lengths {lens[0]} .. {lens[-1]} x 3 rows, worst "
             f"|y - fp64 oracle| {worst:.2e} x max|x| at n = {at}, impulses {worst_imp:.2e} "
             f"(bar {MC.RESAMPLE_BAR:g})")
    assert worst <= MC.RESAMPLE_BAR, (worst, at)
    assert worst_imp <= MC.RESAMPLE_BAR, worst_imp


@pytest.mark.parametrize("orig,new", PAIRS, ids=PAIR_IDS)
def test_no_access_outside_the_arguments(pkg, dev, melmod, orig, new):
    """hfg_resample_forward on slices of larger device tensors: x between 1e30 guards, y
    pre-filled with NaN between NaN guards.  y comes back without a NaN and bitwise the plain
    call's (the zero pad is made by the kernel, never read), and no guard has moved."""
    rs = melmod.Resample(orig, new, device=dev)
    lib = pkg.load_library()
    for n in MC.resample_lengths(orig, new):
        x = torch.from_numpy(np.array(MC.resample_rows(n, orig))).to(dev)
        plain = rs(x)
        n_out = plain.shape[-1]
        xbuf = torch.full((3 * n + 2 * GUARD,), 1e30, device=dev)
        xv = xbuf[GUARD:GUARD + 3 * n]
        xv.copy_(x.reshape(-1))
        ybuf = torch.full((3 * n_out + 2 * GUARD,), float("nan"), device=dev)
        yv = ybuf[GUARD:GUARD + 3 * n_out]
        rc = lib.hfg_resample_forward(rs.ptr, ctypes.c_void_p(xv.data_ptr()), 3, n,
                                      ctypes.c_void_p(yv.data_ptr()),
                                      ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        assert rc == 0, lib.hfg_mel_last_error()
        torch.cuda.synchronize()
        assert not bool(torch.isnan(yv).any()), n
        assert torch.equal(yv.reshape(plain.shape), plain), n
        assert bool((xbuf[:GUARD] == 1e30).all()) and bool((xbuf[GUARD + 3 * n:] == 1e30).all())
        assert torch.equal(xv, x.reshape(-1))
        assert bool(torch.isnan(ybuf[:GUARD]).all()) and bool(torch.isnan(ybuf[GUARD + 3 * n_out:]).all()), n
