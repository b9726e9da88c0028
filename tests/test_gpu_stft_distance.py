"""metrics.MultiResolutionSTFT on the GPU (csrc/spectral_distance.hip, stft_distance_fft)
against the float64 oracle tests/spectral_distance_oracle.py and the reference's recorded
compute_stft_loss (tests/golden/specdist_ref.json).

Bars (derived; the measured maxima go through `evidence`): each side's ln(|X| + eps) lies in
[ln 1e-5, 16) = [-11.6, 16) and is rounded to float32 once, at most 2^-21 each, the float64 FFT
adds orders of magnitude less: |l1 - oracle| <= 2e-6 per item and batch, and
|l2 - oracle| <= 2e-6 (2 l1_oracle + 2e-6).

Measured on an MI355X: max |l1 - oracle| 1.9e-8 (the (64, 24, 40) ragged case; 1.7e-9 at the
reference resolutions), l2 at most 0.015 of its bar; against the reference's recorded loss
1.9e-5 (L1) and 3.5e-4 (L2).  The device window is torch.hann_window's float32 one: with the
double-evaluated window the chirp's L1 is 1.4e-5 off at (1024, 120, 600)."""
import ctypes
import importlib
import json
import os

import numpy as np
import pytest
import torch

import spectral_distance_oracle as O
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu
BAR = 2e-6
N = 8269
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def metrics(pkg):
    return importlib.import_module("tts_sambert_hifigan_amd.metrics")


@pytest.fixture(scope="module")
def ab():
    return O.inputs(N)


@pytest.fixture(scope="module")
def mrstft(metrics, dev):
    return metrics.MultiResolutionSTFT(device=dev)


def host(d):
    return d.sum_abs.cpu().numpy(), d.sum_sq.cpu().numpy(), d.frames.cpu().numpy()


def same_bits(x, y):
    return np.array_equal(np.asarray(x, np.float64).view(np.uint64),
                          np.asarray(y, np.float64).view(np.uint64))


def check(d, a, b, res, lengths, evidence, tag):
    o1, o2, of = O.stft_distance64(a, b, *res, lengths=lengths)
    rows = res[0] // 2 + 1
    assert d.rows == rows and d.frames.cpu().numpy().tolist() == of.tolist(), tag
    p1, p2, l1, l2 = O.means(o1, o2, of, rows)
    g1, g2 = d.per_item_l1.cpu().numpy(), d.per_item_l2.cpu().numpy()
    e1 = max(np.abs(g1 - p1).max(), abs(d.l1.item() - l1))
    r2 = max((np.abs(g2 - p2) / (BAR * (2 * p1 + BAR))).max(),
             abs(d.l2.item() - l2) / (BAR * (2 * l1 + BAR)))
    evidence(f"{tag}: max|l1 - oracle| = {e1:.2e} (bar {BAR:g}), l2 error / its bar = {r2:.3f}; "
             f"l1 {l1:.6f} l2 {l2:.6f}")
    assert e1 <= BAR, (tag, e1)
    assert r2 <= 1.0, (tag, r2)


def test_reference_resolutions(mrstft, dev, ab, evidence):
    a, b = ab
    out = mrstft(a.to(dev), b.to(dev))
    assert len(out) == 3
    for d, res in zip(out, O.RESOLUTIONS):
        assert d.sum_abs.dtype == torch.float64 and d.sum_abs.is_cuda and d.sum_abs.shape == (3,)
        assert d.frames.dtype == torch.int32
        check(d, a, b, res, None, evidence, f"stft {res}")
    with open(os.path.join(GOLDEN_DIR, "specdist_ref.json")) as f:
        gold = json.load(f)
    m1, m2 = gold["measured_max_diff"]["l1"], gold["measured_max_diff"]["l2"]
    e1 = abs(out.l1.item() - gold["overall"]["sc_loss"])
    e2 = abs(out.l2.item() - gold["overall"]["mag_loss"])
    evidence(f"MultiResolutionSTFT vs the reference's recorded loss: |l1 - sc_loss| = {e1:.2e} "
             f"(margin {4 * m1:.2e}), |l2 - mag_loss| = {e2:.2e} (margin {4 * m2:.2e})")
    assert e1 <= 4 * m1 and e2 <= 4 * m2
    for d, rec in zip(out, gold["resolutions"]):
        assert abs(d.l1.item() - rec["sc_loss"]) <= 4 * m1
        assert abs(d.l2.item() - rec["mag_loss"]) <= 4 * m2
    # [B, 1, N], the Generator's output layout
    out3 = mrstft(a[:, None].to(dev), b[:, None].to(dev))
    assert all(same_bits(host(x)[0], host(y)[0]) for x, y in zip(out, out3))


def test_ragged(metrics, dev, ab, evidence):
    """n_fft 2048: lengths [8269, 3000, 1100, 1024] give [35, 13, 5, 0] frames (1024 is not
    more than n_fft / 2); NaN past each length; every item bitwise its solo call."""
    a, b = ab
    lens, frames = [8269, 3000, 1100, 1024], [35, 13, 5, 0]
    a4 = torch.cat([a, a[:1]]).clone()
    b4 = torch.cat([b, b[1:2]]).clone()
    for i, n in enumerate(lens):
        a4[i, n:] = float("nan")
        b4[i, n:] = float("nan")
    one = metrics.MultiResolutionSTFT(resolutions=[(2048, 240, 1200)], device=dev)
    da, db = a4.to(dev), b4.to(dev)
    d = one(da, db, lens)[0]
    s1, s2, fr = host(d)
    assert fr.tolist() == frames
    assert np.isfinite(s1).all() and np.isfinite(s2).all()
    assert s1[3] == 0.0 and s2[3] == 0.0 and d.per_item_l1.tolist()[3] == 0.0
    check(d, a4, b4, (2048, 240, 1200), lens, evidence, "stft 2048 ragged")
    for i, n in enumerate(lens[:3]):
        solo = host(one(da[i:i + 1, :n].contiguous(), db[i:i + 1, :n].contiguous())[0])
        assert solo[2].tolist() == [frames[i]]
        assert same_bits(solo[0], s1[i:i + 1]) and same_bits(solo[1], s2[i:i + 1]), i
    dd = host(one(da, db, torch.tensor(lens, dtype=torch.int32, device=dev))[0])
    assert same_bits(dd[0], s1) and same_bits(dd[1], s2) and dd[2].tolist() == frames
    # device lengths out of range are clamped into [0, N]
    clean_a, clean_b = torch.nan_to_num(da, nan=0.5), torch.nan_to_num(db, nan=0.25)
    wild = torch.tensor([10 ** 9, -4, 1100, 0], dtype=torch.int32, device=dev)
    w = host(one(clean_a, clean_b, wild)[0])
    c = host(one(clean_a, clean_b, [N, 0, 1100, 0])[0])
    assert w[2].tolist() == c[2].tolist() == [35, 0, 5, 0]
    assert same_bits(w[0], c[0]) and same_bits(w[1], c[1])


def test_identical_signals_give_exact_zero(mrstft, dev, ab):
    a, _ = ab
    x = a.to(dev)
    for d in mrstft(x, x):
        assert d.sum_abs.tolist() == [0.0] * 3 and d.sum_sq.tolist() == [0.0] * 3
        assert (d.frames > 0).all()
    out = mrstft(x, x)
    assert out.l1.item() == 0.0 and out.l2.item() == 0.0


@pytest.mark.parametrize("res", [(64, 24, 40), (16, 4, 16)])
def test_small_geometries(metrics, dev, ab, evidence, res):
    """Radix-8 + radix-4 (n_fft 64) and a single radix-8 pass (n_fft 16), a window shorter than
    n_fft, two frames per wave: 8 frames per block.  Lengths chosen so that the frame count
    n // hop + 1 is 0 and 1 modulo 8."""
    a, b = ab
    n_fft, hop, win = res
    one = metrics.MultiResolutionSTFT(resolutions=[res], device=dev)
    for frames in (40, 41):
        n = (frames - 1) * hop + hop // 2
        assert n // hop + 1 == frames and frames % 8 == frames - 40
        d = one(a[:, :n].contiguous().to(dev), b[:, :n].contiguous().to(dev))[0]
        assert d.frames.tolist() == [frames] * 3
        check(d, a[:, :n], b[:, :n], res, None, evidence, f"stft {res} N={n} ({frames} frames)")
    # ragged at the shortest legal length: n_fft / 2 + 1 samples
    n = 39 * hop + 1
    lens = [n, n_fft // 2 + 1, n_fft // 2]
    d = one(a[:, :n].contiguous().to(dev), b[:, :n].contiguous().to(dev), lens)[0]
    assert d.frames.tolist() == [40, (n_fft // 2 + 1) // hop + 1, 0]
    check(d, a[:, :n], b[:, :n], res, lens, evidence, f"stft {res} ragged {lens}")


def test_guards_and_repeat(pkg, metrics, dev, ab):
    """The C ABI on sentinel-filled buffers, and a repeated call bitwise."""
    lib = pkg.load_library()
    a, b = ab
    one = metrics.MultiResolutionSTFT(resolutions=[(1024, 120, 600)], device=dev)
    h = one._dists[0]
    da, db = a.to(dev), b.to(dev)
    first = host(one(da, db)[0])
    again = host(one(da, db)[0])
    assert same_bits(first[0], again[0]) and same_bits(first[1], again[1])
    need = lib.hfg_stftdist_workspace_bytes(h.ptr, 3, N)
    nblk = -(-(N // 120 + 1) // 8)
    assert need == 3 * nblk * 16
    nd = need // 8
    sums = torch.full((GUARD + 6 + GUARD,), -7.5, dtype=torch.float64, device=dev)
    frames = torch.full((GUARD + 3 + GUARD,), -99, dtype=torch.int32, device=dev)
    ws = torch.full((GUARD + nd + GUARD,), -7.5, dtype=torch.float64, device=dev)
    p = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off * x.element_size())
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    args = (h.ptr, p(da), p(db), 3, N, None, p(ws, GUARD))
    assert lib.hfg_stftdist_forward(*args, need - 1, p(sums, GUARD), p(frames, GUARD), st) == -22
    assert lib.hfg_stftdist_forward(*args, need, p(sums, GUARD), p(frames, GUARD), st) == 0
    torch.cuda.synchronize()
    for buf, n, fill in ((sums, 6, -7.5), (frames, 3, -99), (ws, nd, -7.5)):
        t = buf.cpu()
        assert (t[:GUARD] == fill).all() and (t[GUARD + n:] == fill).all()
        assert (t[GUARD:GUARD + n] != fill).all()
    got = sums[GUARD:GUARD + 6].view(3, 2).cpu().numpy()
    assert same_bits(got[:, 0], first[0]) and same_bits(got[:, 1], first[1])
    assert lib.hfg_stftdist_forward(h.ptr, p(da), p(db), 0, N, None, p(ws, GUARD), need,
                                    p(sums, GUARD), p(frames, GUARD), st) == -22
    assert lib.hfg_stftdist_forward(h.ptr, p(da), p(db), 3, 512, None, p(ws, GUARD), need,
                                    p(sums, GUARD), p(frames, GUARD), st) == -22
    with pytest.raises(RuntimeError):
        one(a, b)                         # CPU tensors
    with pytest.raises(RuntimeError):
        one(da, db[:, :100].contiguous())
    with pytest.raises(pkg.HfgError):
        metrics.MultiResolutionSTFT(resolutions=[(1000, 120, 600)], device=dev)
