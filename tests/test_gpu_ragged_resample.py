"""hfg_resample_ragged / mel.Resample.ragged and glue.resynthesize_pcm's resampling on the GPU
(csrc/resample.hip), on the cases of tests/ragged_resample_cases.py.

Bars.  One channel: bitwise the existing kernel (mel.Resample.__call__, resample_sinc) on the
item cropped to its own length: the same fp32 fma chain in the same tap order.  Several channels:
bitwise ((r0 + r1) + ...) / float32(C) formed in numpy fp32 from the existing kernel's
per-channel results (fp32 addition and division are correctly rounded on both sides), and within
mel_cases.RESAMPLE_BAR x max|x| of the float64 reference ragged_ref.  int16 input: bitwise the
float32 run on s / 32768.  No bar is new.

Every input is a dense view into a larger allocation between guards (test_gpu_pcm.guarded), with
NaN (float32) or 32767 (int16) at and past each item's length in every channel; y is pre-filled
with NaN between NaN guards.  A read past a length shows as NaN or as a wrong value, never as an
access outside an allocation; an output that is not written stays NaN."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import mel_cases as MC
import ragged_resample_cases as RC
from test_gpu_pcm import GUARD, chain, guarded  # noqa: F401  (chain: the small release Generator)

pytestmark = pytest.mark.gpu

ALL_PAIRS = RC.PAIRS + [RC.IDENTITY]
ALL_IDS = RC.PAIR_IDS + ["22050-22050"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def melmod(pkg):
    return importlib.import_module("tts_sambert_hifigan_amd.mel")


@pytest.fixture(scope="module")
def pcmmod(pkg):
    return importlib.import_module("tts_sambert_hifigan_amd.pcm")


def poison_of(x):
    return 32767 if x.dtype == np.int16 else float("nan")


def place(x, lens, dev):
    """x numpy [B, C, N] -> ([B, C, N] device view between guards, the whole buffer, a host copy
    of the whole buffer): every channel row carries the poison from lens[b] on."""
    B, C, N = x.shape
    view, big = guarded(np.array(x).reshape(B * C, N), [ln for ln in lens for _ in range(C)],
                        dev, poison_of(x))
    return view.view(B, C, N), big, big.cpu().clone()


def run_c(pkg, rs, view, lens_t):
    """hfg_resample_ragged into a NaN-filled y between NaN guards -> (y view [B, n_out], the
    whole y buffer, out_lengths)."""
    lib = pkg.load_library()
    B, C, N = view.shape
    n_out = rs.out_len(N)
    ybuf = torch.full((2 * GUARD + B * n_out,), float("nan"), device=view.device)
    y = ybuf[GUARD:GUARD + B * n_out].view(B, n_out)
    ol = torch.full((B,), -1, dtype=torch.int32, device=view.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.hfg_resample_ragged(rs.ptr, p(view), 0 if view.dtype == torch.int16 else 1, B, C, N,
                                 p(lens_t) if lens_t is not None else None, p(y), p(ol),
                                 ctypes.c_void_p(torch.cuda.current_stream(view.device).cuda_stream))
    assert rc == 0, lib.hfg_mel_last_error()
    torch.cuda.synchronize()
    return y, ybuf, ol


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and \
        np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_frame(y, ybuf, ol, big, big_host, lens, orig, new, N):
    """Everything about a result but its values inside the lengths: zeros from out_len_b on, no
    NaN, out_lengths, untouched guards and input."""
    n_out = MC.out_len(orig, new, N)
    want_ol = [MC.out_len(orig, new, ln) for ln in lens]
    assert ol.tolist() == want_ol
    yh = y.cpu().numpy()
    assert yh.shape == (len(lens), n_out) and not np.isnan(yh).any()
    for b, m in enumerate(want_ol):
        assert not yh[b, m:].any(), b
    assert bool(torch.isnan(ybuf[:GUARD]).all()) and bool(torch.isnan(ybuf[-GUARD:]).all())
    bh = big.cpu()
    assert torch.equal(bh.view(torch.int16 if bh.dtype == torch.int16 else torch.int32),
                       big_host.view(torch.int16 if bh.dtype == torch.int16 else torch.int32))
    return yh


@pytest.mark.parametrize("orig,new", ALL_PAIRS, ids=ALL_IDS)
def test_float32_against_the_existing_kernel(pkg, dev, melmod, evidence, orig, new):
    """C = 1: bitwise Resample(orig, new)(x[b, :len_b]) per item (identity rates: x itself).
    C = 2, 3, 8: bitwise the numpy fp32 channel mean of the existing kernel's per-channel results
    and within the bar of ragged_ref.  Host lengths through the Python layer give the same bits."""
    rs = melmod.Resample(orig, new, device=dev)
    x = RC.signal(orig, new)
    N, scale = x.shape[-1], float(np.abs(x).max())
    worst = 0.0
    for lens in RC.batches(orig, new):
        lens_t = torch.tensor(lens, dtype=torch.int32, device=dev)
        # the existing kernel on every channel of every cropped item, once: [8, out_len_b]
        per_channel = []
        for b, ln in enumerate(lens):
            if ln == 0:
                per_channel.append(np.zeros((RC.MAX_CHANNELS, 0), np.float32))
                continue
            crop = torch.from_numpy(np.array(x[b, :, :ln])).to(dev)
            r = rs(crop).cpu().numpy()
            assert r.shape == (RC.MAX_CHANNELS, MC.out_len(orig, new, ln))
            per_channel.append(r)
        for C in RC.CHANNELS:
            view, big, big_host = place(np.ascontiguousarray(x[:, :C]), lens, dev)
            y, ybuf, ol = run_c(pkg, rs, view, lens_t)
            yh = check_frame(y, ybuf, ol, big, big_host, lens, orig, new, N)
            for b, r in enumerate(per_channel):
                want = RC.mean_f32(r[:C])
                assert same_bits(yh[b, :want.shape[0]], want), (lens, C, b)
            ref = RC.ragged_ref(x[:, :C], lens, orig, new)
            worst = max(worst, float(np.abs(yh - ref).max()) / scale)
            arg = view[:, 0] if C == 1 else view
            y_py, ol_py = rs.ragged(arg, lens)
            assert y_py.dtype == torch.float32 and ol_py.dtype == torch.int32 and ol_py.is_cuda
            assert torch.equal(ol_py, ol) and same_bits(y_py.cpu().numpy(), yh), (lens, C)
    evidence(f"ragged resample {orig}->{new}: {len(RC.batches(orig, new))} batches x C = "
             f"{RC.CHANNELS}, worst |y - fp64 reference| {worst:.2e} x max|x| "
             f"(bar {MC.RESAMPLE_BAR:g})")
    assert worst <= MC.RESAMPLE_BAR


@pytest.mark.parametrize("orig,new", ALL_PAIRS, ids=ALL_IDS)
def test_int16_is_the_float32_run_on_s_over_32768(pkg, dev, melmod, orig, new):
    rs = melmod.Resample(orig, new, device=dev)
    s = RC.signal_s16(orig, new)
    f = s.astype(np.float32) / np.float32(32768)
    N = s.shape[-1]
    for lens in RC.batches(orig, new):
        lens_t = torch.tensor(lens, dtype=torch.int32, device=dev)
        for C in RC.CHANNELS:
            vi, bi, bi_host = place(np.ascontiguousarray(s[:, :C]), lens, dev)
            vf, bf, bf_host = place(np.ascontiguousarray(f[:, :C]), lens, dev)
            yi, ybi, oli = run_c(pkg, rs, vi, lens_t)
            yf, ybf, olf = run_c(pkg, rs, vf, lens_t)
            a = check_frame(yi, ybi, oli, bi, bi_host, lens, orig, new, N)
            b = check_frame(yf, ybf, olf, bf, bf_host, lens, orig, new, N)
            assert same_bits(a, b), (lens, C)
            assert np.abs(a).max() > 0


@pytest.mark.parametrize("orig,new", ALL_PAIRS, ids=ALL_IDS)
def test_each_item_is_its_solo_run(dev, melmod, orig, new):
    """Item b of a batch is bitwise the B = 1 call on x[b, :, :len_b] with n_samples = len_b."""
    rs = melmod.Resample(orig, new, device=dev)
    for x in (RC.signal(orig, new), RC.signal_s16(orig, new)):
        for lens in RC.batches(orig, new)[:3]:
            for C in (1, 3):
                view, _, _ = place(np.ascontiguousarray(x[:, :C]), lens, dev)
                y, ol = rs.ragged(view, torch.tensor(lens, dtype=torch.int32, device=dev))
                for b, ln in enumerate(lens):
                    if ln == 0:
                        assert ol[b].item() == 0 and not y[b].any()
                        continue
                    solo, sol = rs.ragged(view[b:b + 1, :, :ln].contiguous())
                    m = MC.out_len(orig, new, ln)
                    assert solo.shape == (1, m) and sol.tolist() == [m]
                    assert torch.equal(solo[0].view(torch.int32), y[b, :m].view(torch.int32)), \
                        (lens, C, b)


@pytest.mark.parametrize("orig,new", [(24000, 22050), (22050, 8000), RC.IDENTITY],
                         ids=["24000-22050", "22050-8000", "22050-22050"])
def test_device_lengths_are_clamped(pkg, dev, melmod, orig, new):
    """Device lengths [N + 7, -3, k] behave as [N, 0, k]; no lengths as [N, N, N]."""
    rs = melmod.Resample(orig, new, device=dev)
    x = RC.signal(orig, new)[:, :2]
    N = x.shape[-1]
    k = RC.batches(orig, new)[0][1]
    view, big, big_host = place(np.ascontiguousarray(x), [N, 0, k], dev)
    wild = torch.tensor([N + 7, -3, k], dtype=torch.int32, device=dev)
    y, ybuf, ol = run_c(pkg, rs, view, wild)
    check_frame(y, ybuf, ol, big, big_host, [N, 0, k], orig, new, N)
    y2, ol2 = rs.ragged(view, [N, 0, k])
    assert torch.equal(ol, ol2) and torch.equal(y.view(torch.int32), y2.view(torch.int32))
    full, fbig, fbig_host = place(np.ascontiguousarray(x), [N, N, N], dev)
    y3, ybuf3, ol3 = run_c(pkg, rs, full, None)
    check_frame(y3, ybuf3, ol3, fbig, fbig_host, [N, N, N], orig, new, N)
    y4, _ = rs.ragged(full, [N, N, N])
    assert torch.equal(y3.view(torch.int32), y4.view(torch.int32))


def test_identity_rates(pkg, dev, melmod):
    """Resample(r, r).ragged: y == x inside each length for one channel (-0.0 comes out as +0.0,
    the documented exception), the fp32 channel mean otherwise; __call__ still returns its
    input."""
    rs = melmod.Resample(*RC.IDENTITY, device=dev)
    x = np.array(RC.signal(*RC.IDENTITY))
    x[:, :, 5] = -0.0
    N = x.shape[-1]
    t = torch.from_numpy(x).to(dev)
    assert rs(t) is t
    for lens in RC.batches(*RC.IDENTITY):
        for C in RC.CHANNELS:
            view, big, big_host = place(np.ascontiguousarray(x[:, :C]), lens, dev)
            y, ybuf, ol = run_c(pkg, rs, view, torch.tensor(lens, dtype=torch.int32, device=dev))
            yh = check_frame(y, ybuf, ol, big, big_host, lens, *RC.IDENTITY, N)
            assert ol.tolist() == lens
            for b, ln in enumerate(lens):
                if ln == 0:
                    continue
                want = RC.mean_f32(x[b, :C, :ln] + np.float32(0))    # + 0: -0.0 -> +0.0
                assert same_bits(yh[b, :ln], want), (lens, C, b)
                if C == 1:
                    assert np.array_equal(yh[b, :ln], x[b, 0, :ln])
                    if ln > 5:
                        assert not np.signbit(yh[b, 5]) and np.signbit(x[b, 0, 5])


def test_argument_errors(dev, melmod):
    rs = melmod.Resample(24000, 22050, device=dev)
    x = torch.zeros(3, 2, 64, dtype=torch.int16, device=dev)
    for bad in ([64, 5], [64, 5, 65], [64, -1, 5], [1.5, 2.0, 3.0]):
        with pytest.raises(RuntimeError):
            rs.ragged(x, bad)
    with pytest.raises(RuntimeError):
        rs.ragged(x, torch.tensor([1, 2], dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError):
        rs.ragged(x.to(torch.int32))
    with pytest.raises(RuntimeError):
        rs.ragged(x[0, 0])
    with pytest.raises(RuntimeError):
        rs.ragged(torch.zeros(1, 9, 64, device=dev))
    with pytest.raises(RuntimeError, match="HIP tensor"):
        rs.ragged(x.cpu())


def test_capture_and_replay(dev, melmod):
    """One ragged call (stereo int16, device lengths) captured on one stream and replayed once
    is bitwise the eager result: the call allocates nothing of its own and never syncs."""
    orig, new = 24000, 22050
    rs = melmod.Resample(orig, new, device=dev)
    lens = RC.batches(orig, new)[0]
    view, _, _ = place(np.ascontiguousarray(RC.signal_s16(orig, new)[:, :2]), lens, dev)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev)
    ey, eol = rs.ragged(view, lens_t)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y, ol = rs.ragged(view, lens_t)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(ol, eol) and ol.tolist() == [MC.out_len(orig, new, n) for n in lens]
    assert torch.equal(y.view(torch.int32), ey.view(torch.int32))
    assert ey.abs().max().item() > 0


# ---- the chain ------------------------------------------------------------------------------
CHAIN_SR, CHAIN_N, CHAIN_LENS = 24000, 9000, [9000, 3300, 450]     # -> 8269, 3032, 414 at 22050


def _stereo(dev):
    g = torch.Generator().manual_seed(24000)
    x = (0.3 * torch.randn(3, 2, CHAIN_N, generator=g)).clamp(-1, 1)
    s = (x * 20000).round().to(torch.int16).numpy()
    return place(s, CHAIN_LENS, dev)[0]


def test_resynthesize_pcm_resamples_in_and_out(pcmmod, melmod, chain, dev):
    glue, front, gen = chain
    hop = front.hop_size
    pcm = _stereo(dev)
    lens_t = torch.tensor(CHAIN_LENS, dtype=torch.int32, device=dev)
    L = [MC.out_len(CHAIN_SR, 22050, n) for n in CHAIN_LENS]
    assert L == [8269, 3032, 414]
    frames = [n // hop for n in L]
    out = glue.resynthesize_pcm(gen, front, pcm, lens_t, normalize=True, sample_rate=CHAIN_SR)
    assert out.dtype == torch.int16 and out.shape == (3, (L[0] // hop) * hop)
    # the steps one by one
    rs = melmod.Resample(CHAIN_SR, 22050, device=dev)
    y, ol = rs.ragged(pcm, lens_t)
    assert ol.tolist() == L
    wav = pcmmod.to_float(y, ol, normalize=True)
    with torch.no_grad():
        mel, fl = front(wav, ol)
        gout = gen(mel, lengths=fl)
    assert fl.tolist() == frames
    assert torch.equal(out, pcmmod.to_pcm16(gout, fl * hop))
    assert out.abs().max().item() > 0
    # host lengths: the same bits
    assert torch.equal(glue.resynthesize_pcm(gen, front, pcm, CHAIN_LENS, normalize=True,
                                             sample_rate=CHAIN_SR), out)
    # each item against its solo run
    for b, (n, f) in enumerate(zip(CHAIN_LENS, frames)):
        solo = glue.resynthesize_pcm(gen, front, pcm[b:b + 1, :, :n].contiguous(), normalize=True,
                                     sample_rate=CHAIN_SR)
        assert solo.shape == (1, f * hop)
        assert torch.equal(out[b:b + 1, :f * hop], solo), b
        assert not out[b, f * hop:].any(), b
    # resampled output: lengths ceil(160 L / 441), samples ragged(Generator output)
    out8 = glue.resynthesize_pcm(gen, front, pcm, lens_t, normalize=True, sample_rate=CHAIN_SR,
                                 out_sample_rate=8000)
    rs8 = melmod.Resample(22050, 8000, device=dev)
    y8, ol8 = rs8.ragged(gout[:, 0], fl * hop)
    want8 = [-(-160 * f * hop // 441) for f in frames]
    assert ol8.tolist() == want8 == [MC.out_len(22050, 8000, f * hop) for f in frames]
    assert out8.shape == (3, rs8.out_len(gout.shape[-1]))
    assert torch.equal(out8, pcmmod.to_pcm16(y8, ol8))
    flat, offsets = glue.resynthesize_pcm(gen, front, pcm, lens_t, normalize=True,
                                          sample_rate=CHAIN_SR, out_sample_rate=8000, packed=True)
    assert offsets.tolist() == [0] + list(np.cumsum(want8))
    assert torch.equal(flat[:sum(want8)], torch.cat([out8[b, :m] for b, m in enumerate(want8)]))
    for b, m in enumerate(want8):
        assert not out8[b, m:].any(), b
    # channels at the model rate: the identity filter mixes down and masks
    mix = glue.resynthesize_pcm(gen, front, pcm, lens_t, normalize=True)
    ym, olm = melmod.Resample(22050, 22050, device=dev).ragged(pcm, lens_t)
    with torch.no_grad():
        melm, flm = front(pcmmod.to_float(ym, olm, normalize=True), olm)
        want_mix = pcmmod.to_pcm16(gen(melm, lengths=flm), flm * hop)
    assert torch.equal(mix, want_mix)


def test_default_arguments_keep_the_parent_path(pcmmod, chain, dev):
    """2-d pcm, no rates (or the model's own): bitwise to_float -> front end -> Generator ->
    to_pcm16 called one by one, which is the parent's resynthesize_pcm."""
    glue, front, gen = chain
    hop = front.hop_size
    pcm = _stereo(dev)[:, 0].contiguous()
    lens = [9000, 3300, 450]
    wav = pcmmod.to_float(pcm, lens, normalize=True)
    with torch.no_grad():
        mel, fl = front(wav, lens)
        want = pcmmod.to_pcm16(gen(mel, lengths=fl), fl * hop)
    assert torch.equal(glue.resynthesize_pcm(gen, front, pcm, lens, normalize=True), want)
    assert torch.equal(glue.resynthesize_pcm(gen, front, pcm, lens, normalize=True,
                                             sample_rate=front.sampling_rate,
                                             out_sample_rate=front.sampling_rate), want)
    full = pcm[0:1]
    with torch.no_grad():
        want_full = pcmmod.to_pcm16(gen(front(pcmmod.to_float(full))), None, "nearest")
    assert torch.equal(glue.resynthesize_pcm(gen, front, full, rounding="nearest"), want_full)
