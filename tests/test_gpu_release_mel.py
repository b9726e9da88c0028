"""The public HiFi-GAN release's mel front end on the GPU (mel.ReleaseMelSpectrogram,
csrc/mel_kernels.hip release_mel_fft) against the float64-spectrum restatement
tests/release_mel_oracle.py::mel_f64, in natural-log units.

Bar: max |device - mel_f64| <= 1e-6, derived, not measured: outputs lie in [-11.52, ~3.3],
so the final float32 rounding is at most 2^-21 ~ 4.8e-7; the float64 FFT, sqrt, projection
and log add orders of magnitude less.  The measured maxima are recorded through `evidence`."""
import importlib

import numpy as np
import pytest
import torch

from release_mel_oracle import LOG_CLIP, V1_JSON, mel_f64, quiet_signal, signals

pytestmark = pytest.mark.gpu
BAR = 1e-6
N_RAGGED, LENS, FRAMES = 8269, [8269, 3000, 385], [32, 11, 1]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def melmod(pkg):
    return importlib.import_module("tts_sambert_hifigan_amd.mel")


@pytest.fixture(scope="module")
def front(melmod, dev):
    return melmod.ReleaseMelSpectrogram(device=dev)


@pytest.fixture(scope="module")
def ragged():
    """wav [3, 8269] with the samples past each length overwritten with NaN (shared, never
    modified)."""
    s = signals(N_RAGGED)
    wav = torch.stack([s[0], s[1], 0.5 * (s[0] + s[1])])
    for b, n in enumerate(LENS):
        wav[b, n:] = float("nan")
    return wav


def _err(got, ref64):
    return np.abs(got.cpu().numpy().astype(np.float64) - ref64).max()


@pytest.mark.parametrize("n", [385, 513, 4173, 8269])
def test_release_mel_vs_f64(front, dev, evidence, n):
    """385: one frame, reflection on both sides inside it, the minimum legal length; 513: two
    frames; 4173: not a multiple of hop, a partly filled last block; 8269: 32 frames,
    several blocks."""
    wav = signals(n)
    got = front(wav.to(dev))
    assert got.shape == (2, 80, n // 256) and got.dtype == torch.float32
    assert front.frames(n) == n // 256
    e = _err(got, mel_f64(wav))
    evidence(f"release mel N={n}: max|device - mel_f64| = {e:.2e}")
    assert e <= BAR


@pytest.mark.parametrize("n_fft,hop,win", [(512, 128, 512), (2048, 512, 2048), (256, 64, 256),
                                           (1024, 256, 800)])
def test_release_mel_other_geometries(melmod, dev, evidence, n_fft, hop, win):
    """Other power-of-two n_fft (radix 8 / 4 / 2 passes, one or two frames per wave) and a
    window shorter than n_fft."""
    wav = signals(7000)
    ext = melmod.ReleaseMelSpectrogram(n_fft=n_fft, hop_size=hop, win_size=win, device=dev)
    got = ext(wav.to(dev))
    ref = mel_f64(wav, dict(n_fft=n_fft, hop_size=hop, win_size=win))
    assert got.shape == ref.shape == (2, 80, 7000 // hop)
    e = _err(got, ref)
    evidence(f"release mel n_fft {n_fft} hop {hop} win {win}: max|device - mel_f64| = {e:.2e}")
    assert e <= BAR


def test_release_mel_quiet_bands(front, dev, evidence):
    """A loud burst, then 1e-4-level noise, then exact zeros: the same bar on every band, and
    the all-zero frames are exactly float32(ln 1e-5)."""
    wav = quiet_signal()
    got = front(wav[None].to(dev)).cpu()[0]
    ref = mel_f64(wav[None])[0]
    assert got.shape == ref.shape == (80, 96)
    e = np.abs(got.numpy().astype(np.float64) - ref)
    quiet = ref < ref.max() - 9.0
    evidence(f"release mel quiet bands ({int(quiet.sum())} entries): max err {e[quiet].max():.2e}; "
             f"all {e.max():.2e}")
    assert quiet.sum() > 1000
    assert e.max() <= BAR
    # frame f reads samples [256 f - 384, 256 f + 640): all zero from f = 66 on
    assert (got[:, 66:].numpy() == LOG_CLIP).all()
    assert (got[:, :64].numpy() > LOG_CLIP).any()


def test_release_mel_ragged(front, dev, ragged):
    """lengths [8269, 3000, 385] with NaN past each length: the frame counts, each item
    bitwise its solo run, the padding columns, no NaN; the same with device lengths."""
    mel, fl = front(ragged.to(dev), LENS)
    assert mel.shape == (3, 80, 32)
    assert fl.dtype == torch.int32 and fl.is_cuda and fl.tolist() == FRAMES
    assert not torch.isnan(mel).any()
    for b, (n, f) in enumerate(zip(LENS, FRAMES)):
        solo = front(ragged[b:b + 1, :n].contiguous().to(dev))
        assert solo.shape == (1, 80, f)
        assert torch.equal(mel[b:b + 1, :, :f], solo), b
        assert (mel[b, :, f:].cpu().numpy() == LOG_CLIP).all(), b
        assert _err(solo, mel_f64(ragged[b:b + 1, :n])) <= BAR
    lens_dev = torch.tensor(LENS, dtype=torch.int32, device=dev)
    mel2, fl2 = front(ragged.to(dev), lens_dev)
    assert torch.equal(mel2, mel) and torch.equal(fl2, fl)


def test_release_mel_device_lengths_are_clamped(front, dev, ragged):
    """A device lengths tensor is not read back: out-of-range values are clamped by the
    kernel ([0, N]; no frame when len <= 384), never read past the item."""
    wav = torch.nan_to_num(ragged, nan=0.25).to(dev)
    lens_dev = torch.tensor([10 ** 9, -7, 384], dtype=torch.int32, device=dev)
    mel, fl = front(wav, lens_dev)
    assert fl.tolist() == [32, 0, 0]
    assert torch.equal(mel[0:1], front(wav[0:1]))
    assert (mel[1:].cpu().numpy() == LOG_CLIP).all()


def test_release_mel_argument_errors(front, dev):
    wav = signals(2000)
    with pytest.raises(RuntimeError):
        front(wav)                                   # a CPU wav
    d = wav.to(dev)
    with pytest.raises(RuntimeError):
        front(d, [2000])                             # lengths of the wrong shape
    with pytest.raises(RuntimeError):
        front(d, torch.tensor([2000, 2000, 2000], dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError):
        front(d, [2000, 384])                        # a host length <= 384
    with pytest.raises(RuntimeError):
        front(d, [2001, 2000])                       # a host length > N
    with pytest.raises(RuntimeError):
        front(d[:, :384])                            # no frame
    with pytest.raises(RuntimeError):
        front(d[0])                                  # not [B, N]


def test_mel_from_release_config(pkg, melmod, front, dev):
    """The V1 config.json values give the explicit constructor's mel; fmax null is
    sampling_rate / 2."""
    ck = importlib.import_module("tts_sambert_hifigan_amd.checkpoint")
    wav = signals(4173)
    a = ck.mel_from_release_config(V1_JSON, device=dev)
    assert torch.equal(a(wav.to(dev)), front(wav.to(dev)))
    assert torch.equal(a.filterbank(), front.filterbank()) and torch.equal(a.window(), front.window())
    assert a.filterbank().shape == (513, 80) and a.window().shape == (1024,)
    full = ck.mel_from_release_config(dict(V1_JSON, fmax=None), device=dev)
    got = full(wav.to(dev))
    assert _err(got, mel_f64(wav, dict(fmax=None))) <= BAR
    assert _err(got, mel_f64(wav, dict(fmax=11025.0))) <= BAR
    assert not torch.equal(got, front(wav.to(dev)))


def test_resynthesize_chain(pkg, melmod, front, dev, ragged, evidence):
    """wav -> release mel -> release V1 Generator on the device, frame lengths passed device
    to device: each item bitwise gen(mel, lengths=frame_lengths), within the loose propagated
    1e-3 of the Generator run on mel_f64 (the bar of test_mel_feeds_vocoder), 0 past
    frames_b * 256."""
    import __graft_entry__ as ge
    glue = importlib.import_module(ge.PKG_NAME + ".glue")
    ck = importlib.import_module(ge.PKG_NAME + ".checkpoint")
    S = importlib.import_module(ge.PKG_NAME + ".synth")
    gen = ck.generator_from_release_config(
        {"resblock": "1", "upsample_rates": [8, 8, 2, 2], "upsample_kernel_sizes": [16, 16, 4, 4],
         "upsample_initial_channel": 512, "resblock_kernel_sizes": [3, 7, 11],
         "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5], [1, 3, 5]]}).eval()
    gen.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v))
                         for k, v in S.random_state_dict(S.V1, seed=5).items()})
    gen = gen.to(dev)
    d = ragged.to(dev)
    out = glue.resynthesize(gen, front, d, LENS)
    assert out.shape == (3, 1, 32 * 256)
    mel, fl = front(d, LENS)
    with torch.no_grad():
        assert torch.equal(out, gen(mel, lengths=fl))
        worst = 0.0
        for b, (n, f) in enumerate(zip(LENS, FRAMES)):
            ref = gen(torch.from_numpy(mel_f64(ragged[b:b + 1, :n])).float().to(dev))
            assert ref.shape == (1, 1, f * 256)
            worst = max(worst, (out[b:b + 1, :, :f * 256] - ref).abs().max().item())
            assert not out[b, :, f * 256:].any()
        # equal lengths: no lengths at all
        full = glue.resynthesize(gen, front, d[0:1])
        assert torch.equal(full, out[0:1])
    torch.cuda.synchronize()
    evidence(f"resynthesize (release V1, ragged): max|chain - gen(mel_f64)| = {worst:.2e} "
             f"(max|wav| {out.abs().max().item():.2e})")
    assert worst <= 1e-3
    with pytest.raises((ValueError, RuntimeError)):
        glue.resynthesize(gen, melmod.ReleaseMelSpectrogram(n_fft=512, hop_size=128, win_size=512,
                                                            device=dev), d)
    with pytest.raises((ValueError, RuntimeError)):
        glue.resynthesize(gen, melmod.ReleaseMelSpectrogram(num_mels=64, device=dev), d)
