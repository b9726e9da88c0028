"""Cases and the numpy restatement of the ragged multi-channel resampler (hfg_resample_ragged,
mel.Resample.ragged) for test_ragged_resample_host.py and test_gpu_ragged_resample.py.  Not a
test module and not a conftest: plain helpers.

Truth: oracle.resample_np.resample (float64 accumulation) run per item and per channel on the
item cropped to its own length, the float64 mean over channels, zeros up to the batch's n_out.
The bar is mel_cases.RESAMPLE_BAR (2e-6 x max|x|), none new: the mean of C values each within the
bar is within the bar, and the fp32 channel sum and division add at most C rounding errors of
6e-8 relative (tests/test_ragged_resample_host.py measures the sum of both on every case).

Every pair of mel_cases.RESAMPLE_PAIRS runs as 3-item batches [N, edge, small]:
  N      the largest of mel_cases.resample_lengths(pair): the batch's n_samples, so n_out is 512 or
         513 and the grid has two or three 256-output blocks per item;
  edge   a length of that list whose output length is one of the pair's block-edge targets
         (mel_cases.OUT_HIT: 255, 256, 257, 511, 512 or 513) below n_out;
  small  0, 1, 2, the filter half-width or one more.
Five batches per pair, so every small length and every edge target of the pair is used.  All
channel counts read the first C channels of one seeded [3, 8, N] array per pair.
"""
import functools
import math

import numpy as np

import mel_cases as MC
from oracle import resample_np as R

PAIRS = list(MC.RESAMPLE_PAIRS)
PAIR_IDS = [f"{o}-{n}" for o, n in PAIRS]
CHANNELS = (1, 2, 3, 8)
MAX_CHANNELS = 8
N_BATCHES = 5
IDENTITY = (22050, 22050)
IDENTITY_N = 600
IDENTITY_BATCHES = [[600, 257, 0], [600, 256, 1], [600, 255, 2]]


def small_lengths(orig, new):
    w = MC.width_of(orig, new)
    return [0, 1, 2, w, w + 1]


def edge_lengths(orig, new):
    """[(target, n)]: the block-edge output lengths below the batch's n_out and the input length
    that gives each."""
    lens = MC.resample_lengths(orig, new)
    n_out = MC.out_len(orig, new, max(lens))
    out = []
    for t, n in sorted(MC.out_edge_lengths(orig, new).items()):
        if MC.out_len(orig, new, n) == t and t < n_out:
            out.append((t, n))
    return out


def batches(orig, new):
    """[[N, edge, small]] x N_BATCHES"""
    if (orig, new) == IDENTITY:
        return [list(b) for b in IDENTITY_BATCHES]
    N = max(MC.resample_lengths(orig, new))
    edges, small = edge_lengths(orig, new), small_lengths(orig, new)
    return [[N, edges[i % len(edges)][1], small[i % len(small)]] for i in range(N_BATCHES)]


def n_samples(orig, new):
    return IDENTITY_N if (orig, new) == IDENTITY else max(MC.resample_lengths(orig, new))


@functools.lru_cache(maxsize=None)
def signal(orig, new):
    """x f32 [3, 8, N] = (0.4 randn).clamp(-1, 1), seeded by the pair.  Shared: never modified."""
    import torch
    g = torch.Generator().manual_seed(7919 * orig + new)
    x = (0.4 * torch.randn(3, MAX_CHANNELS, n_samples(orig, new), generator=g)).clamp(-1, 1).numpy()
    x.setflags(write=False)
    return x


def signal_s16(orig, new):
    """The same signal as int16 [3, 8, N] (round(x * 32767))."""
    return np.round(signal(orig, new) * 32767.0).astype(np.int16)


def out_len(orig, new, n):
    return MC.out_len(orig, new, n)


def ragged_ref(x, lengths, orig, new, past=0, ch0_only=False, div_off=0, full_len=False):
    """x [B, C, N] or [B, N] (float) -> float64 [B, n_out].  The keyword hooks are the mutants of
    the host test, each a fault the kernel could have: past = 1 filters one sample beyond the
    item's length (its output length unchanged), ch0_only drops every channel but the first,
    div_off = 1 divides the channel sum by C - 1, full_len takes every item at n_samples."""
    x = np.asarray(x)
    if x.ndim == 2:
        x = x[:, None]
    B, C, N = x.shape
    n_out = MC.out_len(orig, new, N)
    y = np.zeros((B, n_out), np.float64)
    for b in range(B):
        ln = N if full_len else int(lengths[b])
        m = MC.out_len(orig, new, ln)
        if ln == 0:
            continue
        read = min(ln + past, N)
        chans = [R.resample(np.ascontiguousarray(x[b, c, :read], np.float32), orig, new)
                 .astype(np.float64)[:m] for c in range(1 if ch0_only else C)]
        y[b, :m] = np.sum(chans, axis=0) / (len(chans) if ch0_only else C - div_off)
    return y


MUTANTS = {
    "one_sample_past_the_length": dict(past=1),
    "channel_0_only": dict(ch0_only=True),
    "divided_by_C_minus_1": dict(div_off=1),
    "batch_length_for_every_item": dict(full_len=True),
}


def chain_ref(x, lengths, orig, new):
    """The kernel's arithmetic on the CPU: mel_cases.fma_chain per channel on the cropped item,
    ((r0 + r1) + ...) / float32(C) in fp32, zeros to n_out.  float32 [B, n_out]."""
    x = np.asarray(x, np.float32)
    if x.ndim == 2:
        x = x[:, None]
    B, C, N = x.shape
    y = np.zeros((B, MC.out_len(orig, new, N)), np.float32)
    for b in range(B):
        ln = int(lengths[b])
        if ln == 0:
            continue
        r = x[b, :, :ln].copy() if orig == new else MC.fma_chain(x[b, :, :ln], orig, new)
        y[b, :r.shape[1]] = mean_f32(r)
    return y


def mean_f32(r):
    """r f32 [C, n] -> ((r0 + r1) + ...) / float32(C), every step rounded to fp32; C = 1: r0."""
    acc = r[0].astype(np.float32)
    for c in range(1, r.shape[0]):
        acc = (acc + r[c]).astype(np.float32)
    return acc if r.shape[0] == 1 else (acc / np.float32(r.shape[0])).astype(np.float32)


def blocks(n):
    return math.ceil(n / 256)
