"""metrics.mel_distance on the GPU (csrc/spectral_distance.hip, mel_distance_fft): the mel of a
wav against a held mel tensor, fused, against the float64 oracles.

Inputs: spectral_distance_oracle.inputs (a, b [3, 8269]); wav = rows of b, target = the
float32 rounding of the oracle mel of a, so only the wav side carries device error.

Bars (derived, the measured maxima go through `evidence`):
* release front end, L1: |l1 - oracle| <= 1e-6 per item and batch: a mean of |d| moves by at
  most the largest per-entry error of the device mel, whose derived bar is 1e-6
  (tests/test_gpu_release_mel.py);
* L2: |l2 - oracle| <= 1e-6 (2 l1_oracle + 1e-6): d^2 moves by at most e (2 |d| + e);
* reference front end (log10): L1 1e-5, its tested per-entry bar (tests/mel_cases.py FFT_BAR);
* fused against unfused on the device's own mel: relative 1e-12 (only the float64 summation
  order differs: n 2^-53 < 3e-13 for 2560 entries); with target = that mel, exactly 0.0.

Measured on an MI355X: release max |l1 - oracle| 2.7e-8 (N = 385), l2 at most 0.048 of its bar;
reference front end 2.4e-9; fused against unfused relative 0 (abs) and 2.3e-16 (sq).
"""
import importlib

import numpy as np
import pytest
import torch

import spectral_distance_oracle as O
from oracle.mel_torch import CONFIG as REF_CONFIG, log_mel64
from release_mel_oracle import mel_f64

pytestmark = pytest.mark.gpu
BAR, REF_BAR = 1e-6, 1e-5
N, LENS, FRAMES = 8269, [8269, 3000, 385], [32, 11, 1]
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def melmod(pkg):
    return importlib.import_module("tts_sambert_hifigan_amd.mel")


@pytest.fixture(scope="module")
def metrics(pkg):
    return importlib.import_module("tts_sambert_hifigan_amd.metrics")


@pytest.fixture(scope="module")
def front(melmod, dev):
    return melmod.ReleaseMelSpectrogram(device=dev)


@pytest.fixture(scope="module")
def ab():
    """(a, b) float32 [3, 8269], shared and never modified."""
    return O.inputs(N)


@pytest.fixture(scope="module")
def ragged(ab):
    """(wav = b with NaN past each length; target [3, 80, 32] = float32 oracle mel of a cropped
    to each length, NaN at columns >= F_b; the float64 oracle mels of the cropped b)."""
    a, b = ab
    wav = b.clone()
    target = torch.full((3, 80, 32), float("nan"))
    mels_b = []
    for i, (n, f) in enumerate(zip(LENS, FRAMES)):
        wav[i, n:] = float("nan")
        target[i, :, :f] = torch.from_numpy(mel_f64(a[i:i + 1, :n])[0]).float()
        mels_b.append(mel_f64(b[i:i + 1, :n])[0])
    return wav, target, mels_b


def host(d):
    """SpectralDistance -> (sum_abs, sum_sq, frames) numpy."""
    return d.sum_abs.cpu().numpy(), d.sum_sq.cpu().numpy(), d.frames.cpu().numpy()


def same_bits(x, y):
    return np.array_equal(np.asarray(x, np.float64).view(np.uint64),
                          np.asarray(y, np.float64).view(np.uint64))


def check_against_oracle(d, mel_wav64, target32, rows, bar, evidence, tag):
    """d: the device's SpectralDistance; mel_wav64 / target32: per item [rows, F_b] arrays."""
    s1, s2, fr = host(d)
    o1 = np.zeros(len(mel_wav64))
    o2 = np.zeros(len(mel_wav64))
    for i, (m, t) in enumerate(zip(mel_wav64, target32)):
        o1[i], o2[i] = O.sums64(m, t)
        assert fr[i] == m.shape[-1], (tag, i, fr)
    p1, p2, l1, l2 = O.means(o1, o2, fr.astype(np.int64), rows)
    g1, g2 = d.per_item_l1.cpu().numpy(), d.per_item_l2.cpu().numpy()
    e1 = max(np.abs(g1 - p1).max(), abs(d.l1.item() - l1))
    r2 = max((np.abs(g2 - p2) / (bar * (2 * p1 + bar))).max(),
             abs(d.l2.item() - l2) / (bar * (2 * l1 + bar)))
    evidence(f"{tag}: max|l1 - oracle| = {e1:.2e} (bar {bar:g}), l2 error / its bar = {r2:.3f}; "
             f"l1 {np.array2string(p1, precision=4)}")
    assert e1 <= bar, (tag, e1)
    assert r2 <= 1.0, (tag, r2)
    return p1


# ---- 1. against the oracle ----------------------------------------------------------------
@pytest.mark.parametrize("n", [385, 513, 4173, 8269])
def test_distance_vs_oracle(metrics, front, dev, ab, evidence, n):
    """385: the minimum legal length, one frame; 513: two frames; 4173: a part-filled block;
    8269: several blocks."""
    a, b = ab
    target = torch.from_numpy(mel_f64(a[:2, :n])).float()
    d = metrics.mel_distance(front, b[:2, :n].contiguous().to(dev), target.to(dev))
    assert d.sum_abs.dtype == torch.float64 and d.sum_abs.is_cuda and d.sum_abs.shape == (2,)
    assert d.frames.dtype == torch.int32 and d.frames.tolist() == [n // 256] * 2 and d.rows == 80
    mw = mel_f64(b[:2, :n])
    check_against_oracle(d, list(mw), list(target.numpy()), 80, BAR, evidence, f"release N={n}")
    # [B, 1, N] is the Generator's output layout
    d3 = metrics.mel_distance(front, b[:2, None, :n].contiguous().to(dev), target.to(dev))
    assert same_bits(host(d3)[0], host(d)[0]) and same_bits(host(d3)[1], host(d)[1])


# ---- 2. fused against unfused -------------------------------------------------------------
def test_fused_vs_unfused(metrics, front, dev, ab, evidence):
    a, b = ab
    wav = b[:2].contiguous().to(dev)
    target = torch.from_numpy(mel_f64(a[:2])).float().to(dev)
    m = front(wav)
    d = metrics.mel_distance(front, wav, target)
    diff = m.double() - target.double()
    u1, u2 = diff.abs().sum((1, 2)), (diff * diff).sum((1, 2))
    r1 = ((d.sum_abs - u1).abs() / u1).max().item()
    r2 = ((d.sum_sq - u2).abs() / u2).max().item()
    evidence(f"fused vs unfused sums on the device's own mel: relative {r1:.2e} (abs), {r2:.2e} (sq)")
    assert r1 <= 1e-12 and r2 <= 1e-12
    z = metrics.mel_distance(front, wav, m)
    assert z.sum_abs.tolist() == [0.0, 0.0] and z.sum_sq.tolist() == [0.0, 0.0]
    assert z.frames.tolist() == [32, 32]


# ---- 3. ragged ----------------------------------------------------------------------------
def test_ragged(metrics, front, dev, ragged, evidence):
    wav, target, mels_b = ragged
    w, t = wav.to(dev), target.to(dev)
    d = metrics.mel_distance(front, w, t, LENS)
    s1, s2, fr = host(d)
    assert fr.tolist() == FRAMES
    assert np.isfinite(s1).all() and np.isfinite(s2).all()
    p1 = check_against_oracle(d, mels_b, [target[i, :, :f].numpy() for i, f in enumerate(FRAMES)],
                              80, BAR, evidence, "release ragged [8269, 3000, 385]")
    # the figures of tests/test_spectral_distance_host.py::test_mel_oracle_sanity, up to the
    # float32 rounding of the target
    assert np.allclose(p1, [0.1028, 3.931, 0.1478], rtol=2e-3)
    for i, n in enumerate(LENS):
        solo = metrics.mel_distance(front, w[i:i + 1, :n].contiguous(), t[i:i + 1])
        o1, o2, of = host(solo)
        assert of.tolist() == [FRAMES[i]]
        assert same_bits(o1, s1[i:i + 1]) and same_bits(o2, s2[i:i + 1]), i
    again = host(metrics.mel_distance(front, w, t, LENS))
    assert same_bits(again[0], s1) and same_bits(again[1], s2)
    lens_dev = torch.tensor(LENS, dtype=torch.int32, device=dev)
    dd = host(metrics.mel_distance(front, w, t, lens_dev))
    assert same_bits(dd[0], s1) and same_bits(dd[1], s2) and dd[2].tolist() == FRAMES


def test_device_lengths_are_clamped_and_empty_items(metrics, front, dev, ragged):
    """Out-of-range device lengths are clamped into [0, N] as the front end clamps them; a
    length of 0 or <= 384 (the reflect pad) gives no frame and sums of exactly 0.0."""
    wav, target, _ = ragged
    w = torch.nan_to_num(wav, nan=0.25).to(dev)
    t = torch.nan_to_num(target, nan=-1.0).to(dev)
    wild = torch.tensor([10 ** 9, -7, 384], dtype=torch.int32, device=dev)
    s1, s2, fr = host(metrics.mel_distance(front, w, t, wild))
    c1, c2, cf = host(metrics.mel_distance(front, w, t, [N, 0, 384]))
    assert fr.tolist() == cf.tolist() == [32, 0, 0]
    assert same_bits(s1, c1) and same_bits(s2, c2)
    assert s1[1:].tolist() == [0.0, 0.0] and s2[1:].tolist() == [0.0, 0.0] and s1[0] > 0
    full = host(metrics.mel_distance(front, w[0:1], t[0:1]))
    assert same_bits(full[0], s1[:1]) and same_bits(full[1], s2[:1])
    # poisoned past the lengths: the empty items read neither the wav nor the target
    s1n, s2n, frn = host(metrics.mel_distance(front, wav.to(dev), target.to(dev),
                                              [LENS[0], 0, 384]))
    assert frn.tolist() == [32, 0, 0] and s1n[1:].tolist() == [0.0, 0.0] and np.isfinite(s1n).all()
    d = metrics.mel_distance(front, w, t, [N, 0, 384])
    assert d.per_item_l1.tolist()[1:] == [0.0, 0.0]


# ---- 4. a target narrower than the wav's frames -----------------------------------------------
def test_target_columns_bound_the_frames(metrics, front, dev, ab):
    """T = 20 < 32 frames: F = 20, the sums are those of the first 20 columns; and in a 32-wide
    target whose columns >= 20 are NaN, an item of 20 frames reads none of them."""
    a, b = ab
    wav = b[:2].contiguous().to(dev)
    target = torch.from_numpy(mel_f64(a[:2])).float().to(dev)
    narrow = target[:, :, :20].contiguous()
    d = metrics.mel_distance(front, wav, narrow)
    assert d.frames.tolist() == [20, 20]
    diff = front(wav)[:, :, :20].double() - narrow.double()
    assert ((d.sum_abs - diff.abs().sum((1, 2))).abs() / d.sum_abs).max().item() <= 1e-12
    assert ((d.sum_sq - (diff * diff).sum((1, 2))).abs() / d.sum_sq).max().item() <= 1e-12
    poisoned = target.clone()
    poisoned[:, :, 20:] = float("nan")
    lens = [20 * 256, 20 * 256 + 255]
    p = metrics.mel_distance(front, wav, poisoned, lens)
    q = metrics.mel_distance(front, wav, narrow, lens)
    assert p.frames.tolist() == [20, 20]
    assert same_bits(host(p)[0], host(q)[0]) and same_bits(host(p)[1], host(q)[1])
    assert np.isfinite(host(p)[0]).all()


# ---- 5. other geometries ------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop,win", [(512, 128, 512), (2048, 512, 2048), (256, 64, 256),
                                           (1024, 256, 800)])
def test_other_geometries(melmod, metrics, dev, ab, evidence, n_fft, hop, win):
    a, b = ab
    n = 7000
    cfg = dict(n_fft=n_fft, hop_size=hop, win_size=win)
    ext = melmod.ReleaseMelSpectrogram(n_fft=n_fft, hop_size=hop, win_size=win, device=dev)
    target = torch.from_numpy(mel_f64(a[:2, :n], cfg)).float()
    d = metrics.mel_distance(ext, b[:2, :n].contiguous().to(dev), target.to(dev))
    assert d.frames.tolist() == [n // hop] * 2
    check_against_oracle(d, list(mel_f64(b[:2, :n], cfg)), list(target.numpy()), 80, BAR, evidence,
                         f"release n_fft {n_fft} hop {hop} win {win}")


# ---- 6. the reference front end -----------------------------------------------------------
def test_reference_front_end(melmod, metrics, dev, ab, evidence):
    a, b = ab
    ref = melmod.MelSpectrogram(device=dev)
    n, lens, frames = 4173, [4173, 1500, 600], [17, 6, 3]
    target = log_mel64(a[:, :n], REF_CONFIG).float()
    d = metrics.mel_distance(ref, b[:, :n].contiguous().to(dev), target.to(dev))
    assert d.frames.tolist() == [17] * 3
    check_against_oracle(d, list(log_mel64(b[:, :n], REF_CONFIG).numpy()), list(target.numpy()),
                         80, REF_BAR, evidence, "reference N=4173")
    wav = b[:, :n].clone()
    tr = torch.full((3, 80, 17), float("nan"))
    mels_b = []
    for i, (m, f) in enumerate(zip(lens, frames)):
        wav[i, m:] = float("nan")
        tr[i, :, :f] = log_mel64(a[i:i + 1, :m], REF_CONFIG)[0].float()
        mels_b.append(log_mel64(b[i:i + 1, :m], REF_CONFIG)[0].numpy())
    w, t = wav.to(dev), tr.to(dev)
    r = metrics.mel_distance(ref, w, t, lens)
    assert r.frames.tolist() == frames
    check_against_oracle(r, mels_b, [tr[i, :, :f].numpy() for i, f in enumerate(frames)], 80,
                         REF_BAR, evidence, "reference ragged [4173, 1500, 600]")
    s1, s2, _ = host(r)
    for i, m in enumerate(lens):
        solo = host(metrics.mel_distance(ref, w[i:i + 1, :m].contiguous(), t[i:i + 1]))
        assert same_bits(solo[0], s1[i:i + 1]) and same_bits(solo[1], s2[i:i + 1]), i
    # at most n_fft / 2 samples: no frame
    e = metrics.mel_distance(ref, w, t, [4173, 512, 0])
    assert e.frames.tolist() == [17, 0, 0] and e.sum_abs.tolist()[1:] == [0.0, 0.0]


def test_dft_path_handle_is_refused(pkg, melmod, metrics, dev, ab):
    a, b = ab
    dft = melmod.MelSpectrogram(n_fft=400, hop_length=100, win_length=400, device=dev)
    n = 2000
    target = torch.zeros(1, 80, n // 100 + 1, device=dev)
    with pytest.raises(pkg.HfgError, match="DFT-GEMM"):
        metrics.mel_distance(dft, b[:1, :n].contiguous().to(dev), target)


# ---- 7. guard words -----------------------------------------------------------------------
def test_nothing_written_outside_the_outputs(pkg, front, dev, ragged):
    """The C ABI on sentinel-filled buffers: sums, frames and exactly workspace_bytes of the
    workspace are written, the words around them are not."""
    import ctypes
    lib = pkg.load_library()
    wav, target, _ = ragged
    w, t = wav.to(dev), target.to(dev)
    lens = torch.tensor(LENS, dtype=torch.int32, device=dev)
    need = lib.hfg_relmel_distance_workspace_bytes(front.ptr, 3, N)
    assert need == 3 * 4 * 16
    nd = need // 8
    sums = torch.full((GUARD + 6 + GUARD,), -7.5, dtype=torch.float64, device=dev)
    frames = torch.full((GUARD + 3 + GUARD,), -99, dtype=torch.int32, device=dev)
    ws = torch.full((GUARD + nd + GUARD,), -7.5, dtype=torch.float64, device=dev)
    p = lambda x, off: ctypes.c_void_p(x.data_ptr() + off * x.element_size())
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    args = (front.ptr, p(w, 0), 3, N, p(lens, 0), p(t, 0), 32, p(ws, GUARD))
    assert lib.hfg_relmel_distance(*args, need - 1, p(sums, GUARD), p(frames, GUARD), st) == -22
    assert b"workspace" in lib.hfg_mel_last_error()
    assert lib.hfg_relmel_distance(*args, need, p(sums, GUARD), p(frames, GUARD), st) == 0
    torch.cuda.synchronize()
    for buf, n, fill in ((sums, 6, -7.5), (frames, 3, -99), (ws, nd, -7.5)):
        h = buf.cpu()
        assert (h[:GUARD] == fill).all() and (h[GUARD + n:] == fill).all()
        assert (h[GUARD:GUARD + n] != fill).all()
    assert frames[GUARD:GUARD + 3].tolist() == FRAMES
    # the partials of blocks past an item's frames are exact zeros
    part = ws[GUARD:GUARD + nd].view(3, 4, 2).cpu()
    assert (part[1, 2:] == 0).all() and (part[2, 1:] == 0).all() and (part[0] > 0).all()
    # refusals: target_cols < 1, B out of range, a length with no frame
    bad = (front.ptr, p(w, 0), 3, N, p(lens, 0), p(t, 0), 0, p(ws, GUARD))
    assert lib.hfg_relmel_distance(*bad, need, p(sums, GUARD), p(frames, GUARD), st) == -22
    bad = (front.ptr, p(w, 0), 0, N, p(lens, 0), p(t, 0), 32, p(ws, GUARD))
    assert lib.hfg_relmel_distance(*bad, need, p(sums, GUARD), p(frames, GUARD), st) == -22
    bad = (front.ptr, p(w, 0), 3, 384, p(lens, 0), p(t, 0), 32, p(ws, GUARD))
    assert lib.hfg_relmel_distance(*bad, need, p(sums, GUARD), p(frames, GUARD), st) == -22


# ---- 8. capture ---------------------------------------------------------------------------
def test_capture_and_replay(metrics, front, dev, ragged):
    """The two launches captured on one stream (a linear chain) and replayed twice: bitwise the
    eager result.  Lengths are a device tensor: nothing is copied from the host."""
    wav, target, _ = ragged
    w, t = wav.to(dev), target.to(dev)
    lens = torch.tensor(LENS, dtype=torch.int32, device=dev)
    eager = host(metrics.mel_distance(front, w, t, lens))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = metrics.mel_distance(front, w, t, lens)
    for _ in range(2):
        captured.sum_abs.zero_()
        captured.sum_sq.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got = host(captured)
        assert same_bits(got[0], eager[0]) and same_bits(got[1], eager[1])
        assert got[2].tolist() == FRAMES


# ---- 9. the glue --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain(pkg, dev, front):
    """(glue, a small release-layout Generator: V1's rates at 128 initial channels, seeded
    random weights)."""
    import __graft_entry__ as ge
    glue = importlib.import_module(ge.PKG_NAME + ".glue")
    ck = importlib.import_module(ge.PKG_NAME + ".checkpoint")
    S = importlib.import_module(ge.PKG_NAME + ".synth")
    cfg = S.GenConfig(upsample_initial_channel=128)
    gen = ck.generator_from_release_config(
        {"resblock": "1", "upsample_rates": cfg.upsample_rates,
         "upsample_kernel_sizes": cfg.upsample_kernel_sizes,
         "upsample_initial_channel": cfg.upsample_initial_channel,
         "resblock_kernel_sizes": cfg.resblock_kernel_sizes,
         "resblock_dilation_sizes": cfg.resblock_dilation_sizes}).eval()
    gen.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v))
                         for k, v in S.random_state_dict(cfg, seed=5).items()})
    return glue, gen.to(dev)


@pytest.fixture
def no_readback(monkeypatch):
    """Inside the returned context every .item() / .tolist() / .cpu() / .numpy() of a device
    tensor raises."""
    import contextlib

    @contextlib.contextmanager
    def guard():
        with monkeypatch.context() as m:
            for name in ("item", "tolist", "cpu", "numpy"):
                orig = getattr(torch.Tensor, name)

                def wrapped(self, *a, _orig=orig, _name=name, **k):
                    if self.is_cuda:
                        raise AssertionError(f"device tensor read back through .{_name}()")
                    return _orig(self, *a, **k)
                m.setattr(torch.Tensor, name, wrapped)
            yield
    return guard


def test_glue(metrics, front, dev, chain, ragged, no_readback):
    """Item 2 has one frame, so 256 output samples: not more than the reflect pad of 384, which
    the front end cannot frame; it compares no frame and its sums are exactly 0.0."""
    glue, gen = chain
    compared = [32, 11, 0]
    wav, _, _ = ragged
    w = wav.to(dev)
    lens_dev = torch.tensor(LENS, dtype=torch.int32, device=dev)
    # copy-synthesis error, ragged, device lengths: no host round trip
    with no_readback():
        out, d = glue.copy_synthesis_error(gen, front, w, lens_dev)
    assert torch.equal(out, glue.resynthesize(gen, front, w, lens_dev))
    mel, fl = front(w, lens_dev)
    sep = metrics.mel_distance(front, out, mel, fl * 256)
    assert fl.tolist() == FRAMES and d.frames.tolist() == compared
    assert same_bits(host(d)[0], host(sep)[0]) and same_bits(host(d)[1], host(sep)[1])
    assert np.isfinite(host(d)[0]).all() and (host(d)[0][:2] > 0).all() and host(d)[0][2] == 0.0
    # host lengths give the same; no lengths: the whole rows
    out_h, d_h = glue.copy_synthesis_error(gen, front, w, LENS)
    assert torch.equal(out_h, out) and same_bits(host(d_h)[0], host(d)[0])
    out1, d1 = glue.copy_synthesis_error(gen, front, w[0:1])
    assert torch.equal(out1, glue.resynthesize(gen, front, w[0:1])) and torch.equal(out1, out[0:1])
    assert same_bits(host(d1)[0], host(d)[0][:1])
    # consistency: vocode a held mel at T = 32, ragged frame lengths on the device
    mel32 = torch.nan_to_num(mel, nan=0.0)
    with no_readback():
        cw, cd = glue.consistency(gen, front, mel32, fl)
    with torch.no_grad():
        assert torch.equal(cw, gen(mel32, lengths=fl))
    csep = metrics.mel_distance(front, cw, mel32, fl * 256)
    assert cd.frames.tolist() == compared
    assert same_bits(host(cd)[0], host(csep)[0]) and same_bits(host(cd)[1], host(csep)[1])
    cw2, cd2 = glue.consistency(gen, front, mel32, FRAMES)
    assert torch.equal(cw2, cw) and same_bits(host(cd2)[0], host(cd)[0])
    cw3, cd3 = glue.consistency(gen, front, mel32[0:1])
    with torch.no_grad():
        assert torch.equal(cw3, gen(mel32[0:1]))
    assert cd3.frames.tolist() == [32] and same_bits(host(cd3)[0], host(cd)[0][:1])


def test_consistency_with_the_reference_front_end(melmod, metrics, dev, chain):
    """mel.MelSpectrogram frames T * hop samples into T + 1 frames: the first T are compared."""
    glue, gen = chain
    ref = melmod.MelSpectrogram(device=dev)
    g = torch.Generator().manual_seed(11)
    mel = torch.randn(1, 80, 32, generator=g).to(dev)
    wav, d = glue.consistency(gen, ref, mel)
    assert wav.shape == (1, 1, 32 * 256) and d.frames.tolist() == [32] and d.rows == 80
    m = ref(wav[:, 0])
    assert m.shape == (1, 80, 33)
    diff = m[:, :, :32].double() - mel.double()
    assert ((d.sum_abs - diff.abs().sum((1, 2))).abs() / d.sum_abs).max().item() <= 1e-12


def test_argument_errors(metrics, front, dev, ab):
    a, b = ab
    wav = b[:2].contiguous().to(dev)
    target = torch.zeros(2, 80, 32, device=dev)
    with pytest.raises(RuntimeError):
        metrics.mel_distance(front, b[:2], target)            # CPU wav
    with pytest.raises(RuntimeError):
        metrics.mel_distance(front, wav, target.cpu())        # CPU target
    with pytest.raises(RuntimeError):
        metrics.mel_distance(front, wav, target[:, :64])      # rows
    with pytest.raises(RuntimeError):
        metrics.mel_distance(front, wav, target[:1])          # batch
    with pytest.raises(RuntimeError):
        metrics.mel_distance(front, wav, target, [N + 1, 5])  # a host length past N
    with pytest.raises(RuntimeError):
        metrics.mel_distance(front, wav, target, [N])         # shape
    with pytest.raises(TypeError):
        metrics.mel_distance(object(), wav, target)
    with pytest.raises(Exception):
        metrics.mel_distance(front, wav[:, :300].contiguous(), target)   # no frame
