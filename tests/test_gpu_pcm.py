"""The release's PCM boundary on the GPU (pcm.peak / to_float / to_pcm16, csrc/pcm.hip) and
glue.resynthesize_pcm against the numpy restatement tests/pcm_oracle.py.

Every bar is exact equality.  to_float with normalisation: IEEE float64 division and product
followed by one rounding to float32 are each correctly rounded on the device as in numpy, so
the results are the same bits (tests/test_pcm_host.py shows a float32 evaluation differs on
> 20 % of these samples).  peak, the plain conversion and the quantiser are exact operations.

Shapes: B = 3, N = 8269 (odd: int16 rows 1 and 2 and the float rows start off the 16-byte
grid, the scalar path) and N = 8272 (every row aligned, the 16-byte path; three blocks per row
with a partly filled last one), LENS = [8269, 3000, 385]: 3000 ends on a vector group, 385 and
8269 end inside one.  Every input is a dense [B, N] view into a larger allocation with a guard
region in front of and behind the batch (32767 for int16, NaN for float), shifted by 0 or 3
elements (3: row 0 is off the 16-byte grid too), and the samples past each length inside a row
carry the same poison: a missing clamp or length check shows as a wrong value, never as an
access outside the allocation.  (Rows of the C ABI are dense, so between two rows the guard IS
the poisoned tail of the first.)"""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from pcm_oracle import (SPECIALS, normalize_ref, pcm_signals, peak_ref, quantize_ref)
from release_mel_oracle import V1_JSON, mel_f64

pytestmark = pytest.mark.gpu
N_ODD, N_ALIGNED, LENS = 8269, 8272, [8269, 3000, 385]
GUARD = 64          # elements: 128 B of int16, 256 B of float, keeps shift 0 on the 16-byte grid
MEL_BAR = 1e-6      # tests/test_gpu_release_mel.py: the float32 rounding of a mel in [-11.52, 3.3]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pcmmod(pkg):
    return importlib.import_module("tts_sambert_hifigan_amd.pcm")


@pytest.fixture(scope="module")
def base():
    """int16 [3, 8269] (shared, never modified): pcm_oracle.pcm_signals."""
    s = pcm_signals(N_ODD)
    s.setflags(write=False)
    return s


def rows_of(base, n):
    """[3, n] from the shared batch: n = 8272 repeats the first samples at the end."""
    return np.concatenate([base, base[:, :n - N_ODD]], axis=1).copy()


def guarded(rows, lens, dev, poison, shift=0, row_poison=None):
    """rows (numpy [B, N]) on the device as a dense view into a poisoned allocation; the
    samples past lens[b] in row b are poisoned as well.  Returns (view, the whole buffer)."""
    B, n = rows.shape
    t = torch.from_numpy(np.ascontiguousarray(rows)).clone()
    for b, ln in enumerate(lens):
        t[b, ln:] = poison if row_poison is None else row_poison
    big = torch.full((GUARD + shift + B * n + GUARD,), poison, dtype=t.dtype)
    lo = GUARD + shift
    big[lo:lo + B * n] = t.reshape(-1)
    big = big.to(dev)
    view = big[lo:lo + B * n].view(B, n)
    assert view.is_contiguous() and view.data_ptr() % 16 == (shift * t.element_size()) % 16
    return view, big


def lens_arg(kind, lens, dev):
    return lens if kind == "host" else torch.tensor(lens, dtype=torch.int32, device=dev)


# ---- 1. peak --------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("n", [N_ODD, N_ALIGNED])
def test_peak_int16(pcmmod, dev, base, n, shift):
    pcm, _ = guarded(rows_of(base, n), LENS, dev, 32767, shift)
    want = np.array([16656, 10000, 10446], np.float32) / np.float32(32768)
    for kind in ("host", "device"):
        got = pcmmod.peak(pcm, lens_arg(kind, LENS, dev))
        assert got.dtype == torch.float32 and got.is_cuda and got.shape == (3,)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), kind
    assert [float(peak_ref(base[b], m)) for b, m in enumerate(LENS)] == want.tolist()
    # no lengths: the whole rows (unpoisoned copy)
    full, _ = guarded(rows_of(base, n), [n] * 3, dev, 32767, shift)
    want_full = [float(peak_ref(r, n)) for r in rows_of(base, n)]
    assert pcmmod.peak(full).tolist() == want_full


def test_peak_of_minus_32768_is_one(pcmmod, dev, base):
    rows = rows_of(base, N_ODD)
    rows[1, LENS[1] - 1] = -32768           # the last sample inside item 1's length
    pcm, _ = guarded(rows, LENS, dev, 32767)
    got = pcmmod.peak(pcm, LENS).tolist()
    assert got == [16656 / 32768, 1.0, 10446 / 32768]


@pytest.mark.parametrize("n", [N_ODD, N_ALIGNED])
def test_peak_float32_nan_stays_in_its_item(pcmmod, dev, base, n):
    rows = (rows_of(base, n) / 32768.0).astype(np.float32)
    want = [float(np.abs(rows[b, :m]).max()) for b, m in enumerate(LENS)]
    clean, _ = guarded(rows, LENS, dev, float("nan"))
    assert pcmmod.peak(clean, LENS).tolist() == want       # NaN past the lengths: not read
    rows[1, 1717] = np.nan
    wav, _ = guarded(rows, LENS, dev, float("nan"))
    got = pcmmod.peak(wav, LENS).cpu().numpy()
    assert np.isnan(got[1]) and got[0] == want[0] and got[2] == want[2]


def test_peak_device_lengths_are_clamped(pcmmod, dev, base):
    n = N_ODD
    pcm, _ = guarded(rows_of(base, n), [n, 0, 385], dev, 32767)
    wild = torch.tensor([n + 7, -3, 385], dtype=torch.int32, device=dev)
    got = pcmmod.peak(pcm, wild)
    assert torch.equal(got, pcmmod.peak(pcm, [n, 0, 385]))
    assert got.tolist() == [16656 / 32768, 0.0, 10446 / 32768]


# ---- 2. to_float ----------------------------------------------------------------------------
def _padded(items, n):
    out = np.zeros((len(items), n), np.float32)
    for b, v in enumerate(items):
        out[b, :len(v)] = v
    return out


def _same_bits(got, want):
    g = got.cpu().numpy()
    assert g.dtype == want.dtype and g.shape == want.shape
    return np.array_equal(g.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("kind", ["host", "device"])
@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("n", [N_ODD, N_ALIGNED])
def test_to_float_int16(pcmmod, dev, base, n, shift, kind):
    rows = rows_of(base, n)
    pcm, _ = guarded(rows, LENS, dev, 32767, shift)
    lens = lens_arg(kind, LENS, dev)
    plain = pcmmod.to_float(pcm, lens)
    assert plain.shape == (3, n) and plain.dtype == torch.float32
    assert _same_bits(plain, _padded([rows[b, :m].astype(np.float32) / np.float32(32768)
                                      for b, m in enumerate(LENS)], n))
    norm = pcmmod.to_float(pcm, lens, normalize=True, gain=0.95)
    assert _same_bits(norm, _padded([normalize_ref(rows[b], m, 0.95) for b, m in enumerate(LENS)], n))
    assert norm.abs().max().item() == np.float32(0.95)
    other = pcmmod.to_float(pcm, lens, normalize=True, gain=0.3)
    assert _same_bits(other, _padded([normalize_ref(rows[b], m, 0.3) for b, m in enumerate(LENS)], n))


@pytest.mark.parametrize("n", [N_ODD, N_ALIGNED])
def test_to_float_no_lengths(pcmmod, dev, base, n):
    rows = rows_of(base, n)
    pcm, _ = guarded(rows, [n] * 3, dev, 32767)
    assert _same_bits(pcmmod.to_float(pcm), rows.astype(np.float32) / np.float32(32768))
    assert _same_bits(pcmmod.to_float(pcm, normalize=True),
                      np.stack([normalize_ref(r, n) for r in rows]))


@pytest.mark.parametrize("kind", ["host", "device"])
@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("n", [N_ODD, N_ALIGNED])
def test_to_float_float32_input(pcmmod, dev, base, n, shift, kind):
    """float32 input against the same formula with v = float64(x); unnormalised it passes
    through, masked by the lengths."""
    rows = (rows_of(base, n) * np.float32(2.5 / 32768)).astype(np.float32)   # peaks above 1 too
    wav, _ = guarded(rows, LENS, dev, float("nan"), shift)
    lens = lens_arg(kind, LENS, dev)
    assert _same_bits(pcmmod.to_float(wav, lens), _padded([rows[b, :m] for b, m in enumerate(LENS)], n))
    got = pcmmod.to_float(wav, lens, normalize=True)
    assert _same_bits(got, _padded([normalize_ref(rows[b], m) for b, m in enumerate(LENS)], n))


def test_to_float_zero_and_empty_items(pcmmod, dev, base):
    """An all-zero item stays all zeros (divisor 1, not 0 / 0), an empty one too; a float32 item
    with a subnormal peak is left undivided."""
    n = N_ALIGNED
    rows = rows_of(base, n)
    rows[1, :LENS[1]] = 0
    pcm, _ = guarded(rows, LENS, dev, 32767)
    got = pcmmod.to_float(pcm, LENS, normalize=True)
    assert not got[1].any() and not torch.isnan(got).any()
    assert _same_bits(got[0:1], _padded([normalize_ref(rows[0], LENS[0])], n))
    empty = pcmmod.to_float(pcm, [LENS[0], 0, LENS[2]], normalize=True)
    assert not empty[1].any() and torch.equal(empty[0], got[0]) and torch.equal(empty[2], got[2])
    tiny = np.finfo(np.float32).tiny
    f = np.zeros((2, 24), np.float32)
    f[0, :3] = [tiny / 2, -tiny / 4, 0]
    f[1, :3] = [tiny, -tiny / 2, 0]
    wav, _ = guarded(f, [24, 24], dev, float("nan"))
    got = pcmmod.to_float(wav, normalize=True, gain=1.0)
    assert _same_bits(got, np.stack([normalize_ref(f[0], 24, 1.0), normalize_ref(f[1], 24, 1.0)]))
    assert got[1, 0].item() == 1.0 and got[0, 0].item() == float(np.float32(tiny / 2))


# ---- 3. to_pcm16 ----------------------------------------------------------------------------
def _tanh_batch(n):
    """tanh of a seeded randn with the eleven special values planted at each item's start, at
    its end and across the 16-byte boundaries after element 16 of the row."""
    g = torch.Generator().manual_seed(7)
    x = torch.tanh(1.5 * torch.randn(3, n, generator=g)).numpy()
    k = len(SPECIALS)
    for b, m in enumerate(LENS):
        x[b, :k] = SPECIALS
        x[b, m - k:m] = SPECIALS[::-1]
        x[b, 14:14 + k] = SPECIALS          # elements 14..24: two 16-byte boundaries inside
    return x


@pytest.mark.parametrize("row_poison", [float("nan"), float("inf")])
@pytest.mark.parametrize("mode", ["trunc", "nearest"])
@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("n", [N_ODD, N_ALIGNED])
def test_to_pcm16(pkg, pcmmod, dev, n, shift, mode, row_poison):
    """Padded and packed against quantize_ref, host and device lengths, each item against its
    solo run.  The guards are NaN; the samples past a length are NaN or +inf (NaN quantises to
    0, which is also the padding: only +inf shows a padded-layout read past the length)."""
    x = _tanh_batch(n)
    wav, _ = guarded(x, LENS, dev, float("nan"), shift, row_poison)
    want = [quantize_ref(x[b, :m], mode) for b, m in enumerate(LENS)]
    assert len(SPECIALS) == 11 and all((w == 32767).any() and (w == -32768).any() for w in want)
    padded = np.zeros((3, n), np.int16)
    for b, w in enumerate(want):
        padded[b, :len(w)] = w
    cumsum = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    for kind in ("host", "device"):
        lens = lens_arg(kind, LENS, dev)
        got = pcmmod.to_pcm16(wav, lens, rounding=mode)
        assert got.dtype == torch.int16 and got.shape == (3, n)
        assert np.array_equal(got.cpu().numpy(), padded), kind
        assert torch.equal(pcmmod.to_pcm16(wav[:, None, :], lens, rounding=mode), got)
        flat, offsets = pcmmod.to_pcm16(wav, lens, rounding=mode, packed=True)
        assert offsets.dtype == torch.int64 and np.array_equal(offsets.cpu().numpy(), cumsum)
        assert flat.dtype == torch.int16
        assert flat.numel() == (sum(LENS) if kind == "host" else 3 * n)
        assert np.array_equal(flat[:sum(LENS)].cpu().numpy(), np.concatenate(want)), kind
    for b, m in enumerate(LENS):
        solo = pcmmod.to_pcm16(wav[b:b + 1, :m].contiguous(), rounding=mode)
        assert np.array_equal(solo.cpu().numpy()[0], want[b]), b
    # the C ABI on a sentinel-filled packed buffer: nothing beyond offsets[B] is written
    lib = pkg.load_library()
    lens_t = torch.tensor(LENS, dtype=torch.int32, device=dev)
    offs = torch.empty(4, dtype=torch.int64, device=dev)
    buf = torch.full((3 * n + GUARD,), 12345, dtype=torch.int16, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.hfg_pcm_offsets(p(lens_t), 3, n, p(offs), st) == 0
    assert lib.hfg_pcm_from_float(p(wav), 3, n, p(lens_t), pkg._lib.PCM_ROUNDINGS[mode], p(offs),
                                  p(buf), st) == 0
    out = buf.cpu().numpy()
    assert np.array_equal(out[:sum(LENS)], np.concatenate(want))
    assert (out[sum(LENS):] == 12345).all()


def test_to_pcm16_no_lengths_and_clamped_lengths(pcmmod, dev):
    n = N_ODD
    x = _tanh_batch(n)
    wav, _ = guarded(x, [n, 0, 385], dev, float("nan"), 0, float("inf"))
    wild = torch.tensor([n + 7, -3, 385], dtype=torch.int32, device=dev)
    got = pcmmod.to_pcm16(wav, wild)
    assert torch.equal(got, pcmmod.to_pcm16(wav, [n, 0, 385]))
    assert not got[1].any() and not got[2, 385:].any()
    flat, offsets = pcmmod.to_pcm16(wav, wild, packed=True)
    assert offsets.tolist() == [0, n, n, n + 385]
    assert torch.equal(flat[:n], got[0]) and torch.equal(flat[n:n + 385], got[2, :385])
    full, _ = guarded(np.nan_to_num(x, nan=0.25, posinf=2.0, neginf=-2.0), [n] * 3, dev,
                      float("nan"))
    a = pcmmod.to_pcm16(full)
    flat, offsets = pcmmod.to_pcm16(full, packed=True)
    assert offsets.tolist() == [0, n, 2 * n, 3 * n] and torch.equal(flat.view(3, n), a)
    assert np.array_equal(a.cpu().numpy(), quantize_ref(full.cpu().numpy()))


def test_argument_errors(pcmmod, dev, base):
    pcm = torch.from_numpy(rows_of(base, N_ODD)).to(dev)
    for bad in ([N_ODD, 5], [N_ODD, 5, N_ODD + 1], [N_ODD, -1, 5], [1.5, 2.0, 3.0]):
        with pytest.raises(RuntimeError):
            pcmmod.peak(pcm, bad)
        with pytest.raises(RuntimeError):
            pcmmod.to_float(pcm, bad)
        with pytest.raises(RuntimeError):
            pcmmod.to_pcm16(pcm.float(), bad)
    with pytest.raises(RuntimeError):
        pcmmod.peak(pcm, torch.tensor([1, 2], dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError):
        pcmmod.to_float(pcm.to(torch.int32))             # neither int16 nor float32
    with pytest.raises(RuntimeError):
        pcmmod.to_pcm16(pcm)                             # int16 into the quantiser
    with pytest.raises(RuntimeError):
        pcmmod.to_float(pcm, normalize=True, gain=float("inf"))
    with pytest.raises(RuntimeError):
        pcmmod.to_float(pcm[0])                          # not [B, N]
    with pytest.raises(RuntimeError):
        pcmmod.to_pcm16(pcm.float(), rounding="floor")


# ---- 4. the chain ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain(pkg, dev):
    """(glue, release front end from V1_JSON, small release Generator with the seeded weights of
    tests/test_gpu_release_mel.py::test_resynthesize_chain)."""
    import __graft_entry__ as ge
    glue = importlib.import_module(ge.PKG_NAME + ".glue")
    ck = importlib.import_module(ge.PKG_NAME + ".checkpoint")
    S = importlib.import_module(ge.PKG_NAME + ".synth")
    front = ck.mel_from_release_config(V1_JSON, device=dev)
    gen = ck.generator_from_release_config(
        {"resblock": "1", "upsample_rates": [8, 8, 2, 2], "upsample_kernel_sizes": [16, 16, 4, 4],
         "upsample_initial_channel": 512, "resblock_kernel_sizes": [3, 7, 11],
         "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5], [1, 3, 5]]}).eval()
    gen.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v))
                         for k, v in S.random_state_dict(S.V1, seed=5).items()})
    return glue, front, gen.to(dev)


def test_resynthesize_pcm_chain(pcmmod, chain, dev, base, evidence):
    glue, front, gen = chain
    n, hop = N_ODD, 256
    frames = [m // hop for m in LENS]
    pcm, _ = guarded(rows_of(base, n), LENS, dev, 32767)
    out = glue.resynthesize_pcm(gen, front, pcm, LENS, normalize=True)
    assert out.dtype == torch.int16 and out.shape == (3, (n // hop) * hop)
    wav = pcmmod.to_float(pcm, LENS, normalize=True)
    steps = pcmmod.to_pcm16(glue.resynthesize(gen, front, wav, LENS), [f * hop for f in frames])
    assert torch.equal(out, steps)
    assert out.abs().max().item() > 0
    mel, fl = front(wav, LENS)
    assert fl.tolist() == frames
    worst = 0.0
    for b, (m, f) in enumerate(zip(LENS, frames)):
        solo = glue.resynthesize_pcm(gen, front, pcm[b:b + 1, :m].contiguous(), normalize=True)
        assert solo.shape == (1, f * hop)
        assert torch.equal(out[b:b + 1, :f * hop], solo), b
        assert not out[b, f * hop:].any(), b
        ref = mel_f64(torch.from_numpy(normalize_ref(base[b], m))[None])
        worst = max(worst, np.abs(mel[b:b + 1, :, :f].cpu().numpy().astype(np.float64) - ref).max())
    evidence(f"mel inside resynthesize_pcm vs mel_f64(normalize_ref): max err {worst:.2e}")
    assert worst <= MEL_BAR
    lens_dev = torch.tensor(LENS, dtype=torch.int32, device=dev)
    assert torch.equal(glue.resynthesize_pcm(gen, front, pcm, lens_dev, normalize=True), out)
    # the other options reach the output stage: packed, nearest, no normalisation, no lengths
    flat, offsets = glue.resynthesize_pcm(gen, front, pcm, LENS, normalize=True, packed=True)
    assert offsets.tolist() == [0] + list(np.cumsum([f * hop for f in frames]))
    assert torch.equal(flat[:int(offsets[-1])],
                       torch.cat([out[b, :f * hop] for b, f in enumerate(frames)]))
    full, _ = guarded(rows_of(base, n), [n] * 3, dev, 32767)
    plain = glue.resynthesize_pcm(gen, front, full[0:1], rounding="nearest")
    assert torch.equal(plain, pcmmod.to_pcm16(glue.resynthesize(gen, front, pcmmod.to_float(full[0:1])),
                                              rounding="nearest"))


# ---- 5. capture -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [N_ODD, N_ALIGNED])
def test_capture_and_replay(pcmmod, dev, base, n):
    """peak -> to_float -> to_pcm16 captured once on one stream (a linear chain) and replayed
    once: bitwise the eager result.  Lengths are a device tensor: nothing is copied from the
    host inside the capture."""
    pcm, _ = guarded(rows_of(base, n), LENS, dev, 32767)
    lens = torch.tensor(LENS, dtype=torch.int32, device=dev)

    def run():
        pk = pcmmod.peak(pcm, lens)
        wav = pcmmod.to_float(pcm, lens, normalize=True)
        return pk, wav, pcmmod.to_pcm16(wav, lens), pcmmod.to_pcm16(wav, lens, packed=True)

    eager = run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    graph.replay()
    torch.cuda.synchronize()
    pk, wav, q, (flat, offsets) = captured
    epk, ewav, eq, (eflat, eoffsets) = eager
    assert torch.equal(pk, epk) and torch.equal(wav, ewav) and torch.equal(q, eq)
    assert torch.equal(offsets, eoffsets)
    assert torch.equal(flat[:sum(LENS)], eflat[:sum(LENS)])
    assert pk.tolist() == [16656 / 32768, 10000 / 32768, 10446 / 32768]
