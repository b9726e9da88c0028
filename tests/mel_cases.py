"""Configurations, lengths, inputs, float64 references and reference mutants of the mel and
resampler shape tests (test_mel_shapes_host.py, test_gpu_mel_shapes.py,
test_gpu_resample_shapes.py).  Not a test module and not a conftest: plain helpers.

What is under test: the reference's extract_mel path on the device away from its one shape
(1024 / 256 / 1024 / 80 slaney, B = 2) — logmel_fft (n_fft a power of two), stft_power_mfma +
mel_log (every other n_fft) and resample_sinc, with their launch code in mel_capi.cpp /
resample_capi.cpp and mel.MelSpectrogram / mel.Resample / mel.extract_mel.

No tolerance is introduced here.  The FFT path keeps test_gpu_mel.py's 1e-5 (log10) on every
band against oracle.mel_torch.log_mel64; the DFT path keeps _check(fft=False)'s 1e-4 (bands
within 2 decades of the item's maximum) and 5e-4 (within 6 decades), taken against log_mel64,
and its inputs have no quieter band (test_mel_shapes_host.py asserts it on the oracle); the
resampler keeps 2e-6 x max|x| against oracle.resample_np.resample and 1e-7 on the kernel table.

Mutants are computed on the float64 restatements alone (mel_variant, resample_variant, which are
bitwise the oracles when nothing is mutated); project code is never made wrong.
"""
import functools
import math

import numpy as np
import torch

from oracle import mel_torch as M
from oracle import resample_np as R

FFT_BAR = 1e-5            # test_gpu_mel.py: every band vs log_mel64
DFT_BAR_STRONG = 1e-4     # _check(fft=False): bands within 2 decades of the item's maximum
DFT_BAR = 5e-4            # ... within 6 decades
DFT_DECADES = 6.0
RESAMPLE_BAR = 2e-6       # x max|x|
KERNEL_BAR = 1e-7


def _cfg(name, n_fft, hop, win, n_mels, **kw):
    c = dict(M.CONFIG, n_fft=n_fft, hop_length=hop, win_length=win, n_mels=n_mels)
    c.update(kw)
    c["name"] = name
    return c


# n_fft / hop / win / n_mels; everything else is the reference's default (22050 Hz, slaney
# scale and norm, 0 .. 8000 Hz)
FFT_CONFIGS = [
    _cfg("1024_256_1024_80", 1024, 256, 1024, 80),
    _cfg("1024_200_800_80", 1024, 200, 800, 80, f_min=55.0, f_max=7600.0),
    _cfg("512_160_400_40_htk", 512, 160, 400, 40, mel_scale="htk", norm=None, sample_rate=16000,
         f_max=8000.0),
    _cfg("2048_512_2048_128", 2048, 512, 2048, 128, f_max=11025.0),
    _cfg("64_64_64_80", 64, 64, 64, 80),          # hop = n_fft; 40 of the 80 bands have no bin
    _cfg("128_96_128_13", 128, 96, 128, 13),
    _cfg("32_8_32_6", 32, 8, 32, 6),
    _cfg("16_4_16_4_htk", 16, 4, 16, 4, mel_scale="htk", f_max=11025.0),
]
DFT_CONFIGS = [
    _cfg("400_160_400_40_htk", 400, 160, 400, 40, mel_scale="htk", norm=None, sample_rate=16000),
    _cfg("1200_300_1200_80", 1200, 300, 1200, 80, sample_rate=24000, f_max=12000.0),
    _cfg("126_32_126_20", 126, 32, 126, 20),      # n_bins = 64 = bins_pad
    _cfg("50_10_50_8", 50, 10, 50, 8),            # 25 trips of the k loop
]
# the DFT path forced at a power of two (schedule knob MEL_DFT = 1, read at handle creation)
DFT_FORCED = _cfg("1024_256_1024_80_forced", 1024, 256, 1024, 80)
EMPTY_BANDS = {"64_64_64_80": 40}
# refused: by the constructor (odd n_fft, win_length > n_fft, n_fft / hop too large for the DFT
# tiles) or by the call (N = n_fft / 2)
REFUSED_CONFIGS = [
    _cfg("odd_n_fft", 1023, 256, 1023, 80),
    _cfg("win_gt_n_fft", 1024, 256, 1025, 80),
    _cfg("dft_too_large", 3000, 750, 3000, 80),
]
EXTRACT_CONFIG = _cfg("extract_1024_200_800", 1024, 200, 800, 80)


def is_pow2(n):
    return n & (n - 1) == 0


def fft_fpb(cfg):
    """Frames per block of logmel_fft: 4 waves x 2 frames, 1 frame at n_fft = 2048."""
    return 8 if cfg["n_fft"] <= 1024 else 4


def frames(cfg, n):
    return n // cfg["hop_length"] + 1


def n_bins(cfg):
    return cfg["n_fft"] // 2 + 1


def shortest(cfg):
    """The shortest accepted length: the left and right reflections meet inside one frame."""
    return cfg["n_fft"] // 2 + 1


def fft_lengths(cfg):
    """Sorted lengths of an FFT configuration: the two shortest, every frame count 1 .. 2 fpb + 1
    (each residue of the block in the first block and in the second) and one sample either
    side of a full first and second block."""
    hop, fpb, lo = cfg["hop_length"], fft_fpb(cfg), shortest(cfg)
    out = {lo, lo + 1}
    out |= {(f - 1) * hop for f in range(1, 2 * fpb + 2)}
    for f in (fpb, 2 * fpb):
        out |= {f * hop - 1, f * hop + 1}
    return sorted(n for n in out if n >= lo)


DFT_FRAME_COUNTS = (15, 16, 17, 31, 32, 33, 64, 65)   # mel_log's 16, stft_power_mfma's 32, a third block
DFT_RAGGED_FRAMES = 20


def dft_lengths(cfg):
    """Sorted lengths of a DFT configuration: the shortest, the block tails of both kernels and
    one N with N % hop = hop - 1."""
    hop = cfg["hop_length"]
    out = {shortest(cfg), DFT_RAGGED_FRAMES * hop - 1}
    out |= {(f - 1) * hop for f in DFT_FRAME_COUNTS}
    return sorted(out)


def lengths(cfg):
    return fft_lengths(cfg) if cfg in FFT_CONFIGS else dft_lengths(cfg)


def guard_lengths(cfg):
    """The lengths of the guard test: the shortest and one block tail."""
    if cfg in FFT_CONFIGS:
        return [shortest(cfg), fft_fpb(cfg) * cfg["hop_length"]]     # fpb + 1 frames
    return [shortest(cfg), 32 * cfg["hop_length"]]                    # 33 frames


# ----------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mel_batch(n, sample_rate):
    """wav f32 [3, n]: tones + noise, quiet noise, louder noise — levels and contents differ per
    item, so a read of the wrong item's samples or table row is loud.  Shared: never modified."""
    g = torch.Generator().manual_seed(1000003 * sample_rate + n)
    t = torch.arange(n, dtype=torch.float64) / sample_rate
    tones = 0.3 * torch.sin(2 * np.pi * 220.0 * t) + 0.2 * torch.sin(2 * np.pi * 0.14 * sample_rate * t)
    return torch.stack([tones.float() + 0.1 * torch.randn(n, generator=g),
                        0.05 * torch.randn(n, generator=g),
                        0.2 * torch.randn(n, generator=g)])


@functools.lru_cache(maxsize=None)
def mel_ref(name, n):
    """(wav [3, n], log_mel64 [3, n_mels, frames] float64) of a configuration at length n."""
    cfg = BY_NAME[name]
    wav = mel_batch(n, cfg["sample_rate"])
    return wav, M.log_mel64(wav, cfg)


@functools.lru_cache(maxsize=None)
def resample_rows(n, seed):
    """x f32 [3, n] = (0.4 randn).clamp(-1, 1), as test_gpu_mel.py's."""
    g = torch.Generator().manual_seed(seed)
    x = (0.4 * torch.randn(3, n, generator=g)).clamp(-1, 1).numpy()
    x.setflags(write=False)
    return x


def impulses(n):
    """x f32 [3, n]: a unit impulse at sample 0, at the middle sample and at sample n - 1; the
    output is the filter's own taps."""
    x = np.zeros((3, n), np.float32)
    x[0, 0] = x[1, n // 2] = x[2, n - 1] = 1.0
    return x


# ----------------------------------------------------------------------------------------
# mel reference with mutation hooks
# ----------------------------------------------------------------------------------------
def mel_variant(wav, cfg, pad="reflect", centred=True, drop_tail_of=0):
    """oracle.mel_torch.log_mel64 restated (bitwise, with the defaults) with three hooks:
    pad = "zero": the reflect pad replaced by a zero pad; centred = False: a window shorter than
    n_fft placed at offset 0; drop_tail_of = fpb: the last frame of a partial block of fpb frames
    is never computed (its spectrum stays zero: log10(eps))."""
    n_fft, hop, win = cfg["n_fft"], cfg["hop_length"], cfg["win_length"]
    w = torch.zeros(n_fft)
    left = (n_fft - win) // 2 if centred else 0
    w[left:left + win] = torch.hann_window(win)
    x = torch.nn.functional.pad(wav[:, None], (n_fft // 2, n_fft // 2),
                                mode="reflect" if pad == "reflect" else "constant")[:, 0]
    n_frames = wav.shape[-1] // hop + 1
    idx = torch.arange(n_frames)[:, None] * hop + torch.arange(n_fft)[None]
    fr = (x[:, idx] * w).numpy().astype(np.float64)
    spec = np.abs(np.fft.rfft(fr, axis=-1)) ** 2
    if drop_tail_of and n_frames % drop_tail_of:
        spec[:, -1] = 0.0
    fb = M.melscale_fbanks(n_fft // 2 + 1, cfg["f_min"], cfg["f_max"], cfg["n_mels"],
                           cfg["sample_rate"], cfg["norm"], cfg["mel_scale"]).numpy().astype(np.float64)
    return torch.from_numpy(np.log10(np.einsum("bfk,km->bmf", spec, fb) + cfg["eps"]))


MEL_MUTANTS = {
    "zero_pad": dict(pad="zero"),
    "tail_frame_dropped": None,          # drop_tail_of = the configuration's block (mel_mutant)
    "window_at_0": dict(centred=False),  # only where win_length < n_fft
}


def block_frames(cfg):
    """Frames per block whose tail the 'tail_frame_dropped' mutant drops: logmel_fft's block on
    the FFT path, mel_log's 16 on the DFT path (stft_power_mfma's 32 is a multiple)."""
    return fft_fpb(cfg) if cfg in FFT_CONFIGS else 16


def mel_mutant(wav, cfg, mutant):
    kw = MEL_MUTANTS[mutant] or dict(drop_tail_of=block_frames(cfg))
    return mel_variant(wav, cfg, **kw)


def mel_mutant_applies(cfg, mutant):
    return mutant != "window_at_0" or cfg["win_length"] < cfg["n_fft"]


def dft_masks(ref64_item):
    """(strong, big) band masks of one item's float64 log-mel: within 2 and within 6 decades of
    its maximum (_check's masks, on the float64 oracle)."""
    top = ref64_item.max()
    return ref64_item >= top - 2.0, ref64_item >= top - DFT_DECADES


# ----------------------------------------------------------------------------------------
# resampler cases
# ----------------------------------------------------------------------------------------
# (orig, new): (phases, stride, klen) of the reduced rates
RESAMPLE_PAIRS = {
    (11025, 22050): (2, 1, 15),
    (8000, 22050): (441, 160, 174),
    (24000, 22050): (147, 160, 174),
    (32000, 22050): (441, 640, 658),
    (96000, 22050): (147, 640, 694),
    (22050, 8000): (160, 441, 475),
    (22050, 24000): (160, 147, 161),
    (2, 3): (3, 2, 16),
    (3, 2): (2, 3, 23),
}
OUT_TARGETS = (255, 256, 257, 511, 512, 513)    # either side of resample_sinc's 256-output blocks
# the targets some input length hits exactly (the others are stepped over: phases / stride > 1
# outputs per input sample); pinned here, recomputed by the host test
OUT_HIT = {
    (11025, 22050): (256, 512),
    (8000, 22050): (257, 513),
    (24000, 22050): (255, 256, 257, 511, 512, 513),
    (32000, 22050): (255, 256, 257, 511, 512, 513),
    (96000, 22050): (255, 256, 257, 511, 512, 513),
    (22050, 8000): (255, 256, 257, 511, 512, 513),
    (22050, 24000): (255, 256, 257, 511, 512, 513),
    (2, 3): (255, 257, 512, 513),
    (3, 2): (255, 256, 257, 511, 512, 513),
}


def reduced(orig, new):
    g = math.gcd(orig, new)
    return orig // g, new // g


def out_len(orig, new, n):
    """oracle.resample_np.resample's output length."""
    o, w = reduced(orig, new)
    return math.ceil(w * n / o)


def width_of(orig, new):
    return R.sinc_kernel(orig, new)[1]


def out_edge_lengths(orig, new):
    """{target: smallest n whose out_len(n) reaches it}"""
    o, w = reduced(orig, new)
    out = {}
    for t in OUT_TARGETS:
        n = max(1, t * o // w - 1)
        while out_len(orig, new, n) < t:
            n += 1
        while n > 1 and out_len(orig, new, n - 1) >= t:
            n -= 1
        out[t] = n
    return out


def out_hit(orig, new):
    return tuple(t for t, n in out_edge_lengths(orig, new).items() if out_len(orig, new, n) == t)


def resample_lengths(orig, new):
    """Sorted input lengths of a pair: 1, 2, the filter half-width and one more, one stride and
    either side of it, and the output-block edges."""
    stride = reduced(orig, new)[0]
    w = width_of(orig, new)
    out = {1, 2, w, w + 1, stride - 1, stride, stride + 1} | set(out_edge_lengths(orig, new).values())
    return sorted(n for n in out if n >= 1)


def resample_variant(x, orig_freq, new_freq, phase_shift=0, left_short=0):
    """oracle.resample_np.resample restated (bitwise, with the defaults) with two hooks:
    phase_shift: output phase j uses kernel row (j + phase_shift) % phases; left_short: the left
    zero pad is that many samples short."""
    orig, new = reduced(orig_freq, new_freq)
    kern, width = R.sinc_kernel(orig_freq, new_freq)
    kern = np.roll(kern, -phase_shift, axis=0)
    x2 = np.asarray(x, np.float64).reshape(-1, x.shape[-1])
    n = x2.shape[1]
    xp = np.pad(x2, ((0, 0), (width - left_short, width + orig + left_short)))
    n_frames = (xp.shape[1] - kern.shape[1]) // orig + 1
    fr = np.lib.stride_tricks.sliding_window_view(xp, kern.shape[1], axis=1)[:, ::orig][:, :n_frames]
    y = np.einsum("bfk,jk->bfj", fr, kern.astype(np.float64)).reshape(x2.shape[0], -1)
    target = math.ceil(new * n / orig)
    return y[:, :target].reshape(x.shape[:-1] + (target,)).astype(np.float32)


RESAMPLE_MUTANTS = {"phase_plus_1": dict(phase_shift=1), "left_pad_short": dict(left_short=1)}


def fma_chain(x, orig_freq, new_freq):
    """resample_sinc's arithmetic on the CPU: for every output one sequential fp32 fma chain over
    the klen taps of its phase on the zero-padded input.  Each fma is the float64 sum of the
    exact product (24 x 24 bits) and the accumulator, rounded to fp32: the fp32 fma but for
    double rounding, which moves a result by at most one fp32 ulp of a partial sum, rarely."""
    orig, new = reduced(orig_freq, new_freq)
    kern, width = R.sinc_kernel(orig_freq, new_freq)
    x2 = np.asarray(x, np.float32).reshape(-1, x.shape[-1])
    n = x2.shape[1]
    n_out = math.ceil(new * n / orig)
    xp = np.pad(x2, ((0, 0), (width, width + orig + kern.shape[1]))).astype(np.float64)
    m = np.arange(n_out)
    q, j = m // new, m % new
    acc = np.zeros((x2.shape[0], n_out), np.float32)
    k64 = kern.astype(np.float64)
    for k in range(kern.shape[1]):
        acc = (xp[:, q * orig + k] * k64[j, k][None] + acc.astype(np.float64)).astype(np.float32)
    return acc


# ----------------------------------------------------------------------------------------
# handles
# ----------------------------------------------------------------------------------------
BY_NAME = {c["name"]: c for c in FFT_CONFIGS + DFT_CONFIGS + [DFT_FORCED, EXTRACT_CONFIG] + REFUSED_CONFIGS}


def class_kwargs(cfg):
    """mel.MelSpectrogram's keyword arguments of a configuration."""
    return dict(sample_rate=cfg["sample_rate"], n_fft=cfg["n_fft"], hop_length=cfg["hop_length"],
                win_length=cfg["win_length"], n_mels=cfg["n_mels"], f_min=cfg["f_min"],
                f_max=cfg["f_max"], mel_scale=cfg["mel_scale"], norm=cfg["norm"])


def c_config(pkg, cfg):
    """HfgMelConfig of a configuration (what mel.MelSpectrogram builds)."""
    c = pkg._lib.HfgMelConfig()
    c.sample_rate, c.n_fft, c.hop_length, c.win_length, c.n_mels = (
        cfg["sample_rate"], cfg["n_fft"], cfg["hop_length"], cfg["win_length"], cfg["n_mels"])
    c.f_min, c.f_max = cfg["f_min"], cfg["f_max"]
    c.mel_scale = {"slaney": 0, "htk": 1}[cfg["mel_scale"]]
    c.norm = 1 if cfg["norm"] == "slaney" else 0
    c.log_eps, c.log_base = cfg["eps"], 10
    return c


def dft_workspace_bytes(cfg, B, n):
    return 4 * B * frames(cfg, n) * n_bins(cfg)
