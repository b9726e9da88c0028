"""Inputs, float64 references and bars of the dynamic-range tests (test_dynamic_range_host.py,
test_gpu_dynamic_range.py).  Not a test module and not a conftest: plain helpers.

What is under test: the f16x3 mode scales every operand by a power of two taken from a
max-abs reduction (csrc/bf16x3_common.h) — per layer for weights (pack.cpp), per launch and
batch item for activations (amax_commit / x3_exp_slot, absmax_kernel for tensors that arrive
from outside), per block and window inside the whole-ResBlock / whole-MRF kernels (wave_amax /
block_exp).  The inputs built here are the ones a flat randn input never produces: one loud
column beside quiet ones, one loud channel, log-mel silence, items of a batch that differ by
2^80 in magnitude, maxima that sit exactly on a power of two, NaN / inf items.

The bar is regional.  A compared tensor is split in time into the HOT region (columns within
the receptive-field radius RF of a spiked column; 2 RF on generator stages and wavs, whose
polyphase upsamplers' zero taps may widen the support) and the QUIET region (the rest), and
the project's stage rule (tests/test_gpu_stages.py) is applied to each region on its own:

    max|hip - ref64| over the region <= max(STAGE_RTOL[p] * max(1, max|ref64| over the region),
                                            4 * cond_region)

with cond_region = max|fp32 oracle - ref64| over the same region.  A whole-tensor bar would
be set by the loud part and could not see the quiet part crushed.  No tolerance constant is
introduced here: STAGE_RTOL is test_gpu_stages.py's.
"""
import functools
from dataclasses import dataclass
from typing import Tuple

import numpy as np
import torch

from oracle import config as C
from oracle import hifigan_np64 as N
from oracle import hifigan_torch as H
from oracle import prng
from release_oracle import block_forward
from test_gpu_stages import STAGE_RTOL  # noqa: F401  (re-exported: the only tolerances used)

CONTROLS = ["f16x3", "bf16x3", "fp32"]   # f16x3 under test; the other two have no scaling


# ----------------------------------------------------------------------------------------
# standalone MRF / ResBlock / ResBlock2 entries (the modules gen.mrfs[i] and
# gen.mrfs[i].resblocks[j] of a Generator are instances of the same classes)
# ----------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Block:
    name: str
    channels: int
    kernels: Tuple[int, ...]
    dilations: Tuple[Tuple[int, ...], ...]
    resblock: str = "1"   # "1": dilation pairs, "2": one conv per dilation
    j: int = -1           # ResBlock j alone, or -1: the whole MRF
    seed: int = 0
    bias: bool = True     # False: zero biases (outputs as small as the inputs stay visible)

    @property
    def blocks(self):
        return range(len(self.kernels)) if self.j < 0 else [self.j]

    def radius(self, j):
        """Receptive-field radius of ResBlock j in columns: the sum of its conv radii."""
        k, dils = self.kernels[j], self.dilations[j]
        r = sum((k - 1) // 2 * d for d in dils)
        return r if self.resblock == "2" else r + (k - 1) // 2 * len(dils)

    @property
    def rf(self):
        return max(self.radius(j) for j in self.blocks)


V1_K, V1_D = (3, 7, 11), ((1, 3, 5),) * 3
V2_K, V2_D = (3, 5, 7), ((1, 2), (2, 6), (3, 12))

# case 1: every whole-block kernel.  V1 stage 1 (C = 128) runs only k = 3 as a whole-ResBlock
# launch (k = 7 / 11 are layer launches there), stages 2 and 3 all three (k = 11 split in two)
SPIKE_BLOCKS = [
    Block("v1s1_k3", 128, V1_K, V1_D, j=0, seed=101),
    Block("v1s2_k3", 64, V1_K, V1_D, j=0, seed=102),
    Block("v1s2_k7", 64, V1_K, V1_D, j=1, seed=102),
    Block("v1s2_k11", 64, V1_K, V1_D, j=2, seed=102),
    Block("v1s3_k3", 32, V1_K, V1_D, j=0, seed=103),
    Block("v1s3_k7", 32, V1_K, V1_D, j=1, seed=103),
    Block("v1s3_k11", 32, V1_K, V1_D, j=2, seed=103),
    Block("v2s3_mrf16", 16, V2_K, V2_D, seed=104),       # mrf_thin_mfma (fp32: mrf_thin)
    Block("v2s4_mrf8", 8, V2_K, V2_D, seed=105),         # mrf_thin
    Block("rb2_c64_k3", 64, V2_K, V2_D, "2", j=0, seed=106),
    Block("rb2_c64_k7", 64, V2_K, V2_D, "2", j=2, seed=106),
]
SPIKE_RATIOS = [2.0 ** 10, 2.0 ** 16]
LIMIT_BLOCK = SPIKE_BLOCKS[1]   # case 5: C = 64, R = 2^30
LIMIT_RATIO = 2.0 ** 30
# case 2: one conv pair, so that S below is the exact first-order sensitivity
OUTLIER_BLOCKS = [Block("pair_c128", 128, (3,), ((1,),), seed=111),
                  Block("pair_c32", 32, (3,), ((1,),), seed=112)]
OUTLIER_GAIN = 2.0 ** 12
# case 4: maxima exactly on / one ulp under a power of two
EXACT_BLOCK = Block("exact_c64_k3", 64, V1_K, V1_D, j=0, seed=121)
EXACT_K = [-3, 0, 9]
# the subnormal grid: one conv (ResBlock2, one dilation), no bias
GRID_BLOCK = Block("grid_rb2_c64", 64, (3,), ((1,),), "2", j=0, seed=122, bias=False)


def block_state(blk):
    """Default-init-bounded PRNG weights under the module's own state_dict keys."""
    sd = {}
    names = ("convs",) if blk.resblock == "2" else ("convs1", "convs2")
    for j, (k, dils) in enumerate(zip(blk.kernels, blk.dilations)):
        bound = 1.0 / np.sqrt(blk.channels * k)
        for n in names:
            for m in range(len(dils)):
                key = f"resblocks.{j}.{n}.{m}"
                sd[key + ".weight"] = prng.uniform_sym(blk.seed, key + ".weight",
                                                       (blk.channels, blk.channels, k), bound)
                sd[key + ".bias"] = prng.uniform_sym(blk.seed, key + ".bias", (blk.channels,),
                                                     bound if blk.bias else 0.0)
    return sd


def block_convs(blk, j):
    """[(state_dict prefix, dilation)] of ResBlock j's convs in execution order."""
    out = []
    for m, d in enumerate(blk.dilations[j]):
        if blk.resblock == "2":
            out.append((f"resblocks.{j}.convs.{m}", d))
        else:
            out += [(f"resblocks.{j}.convs1.{m}", d), (f"resblocks.{j}.convs2.{m}", 1)]
    return out


def make_module(pkg, blk, precision, dev):
    """The HIP module of the entry and the callable that runs it."""
    mrf = pkg.MRF(blk.channels, list(blk.kernels), [list(d) for d in blk.dilations],
                  precision=precision, resblock=blk.resblock).eval()
    mrf.load_state_dict({k: torch.from_numpy(v) for k, v in block_state(blk).items()})
    mrf = mrf.to(dev)
    return mrf if blk.j < 0 else mrf.resblocks[blk.j]


@functools.lru_cache(maxsize=None)
def block_windows(pkg, blk):
    """[(W, halo)] of the whole-block launches the f16x3 plan runs for this entry, read from
    hfg_debug_plan on a host-only handle (a split ResBlock: one pair per part).  The default
    schedule's: a caller that overrides the schedule asks before it does."""
    assert not pkg.schedule_overrides(), "window geometry is the default schedule's"
    ks = list(blk.kernels) if blk.j < 0 else [blk.kernels[blk.j]]
    ds = [list(d) for d in blk.dilations] if blk.j < 0 else [list(blk.dilations[blk.j])]
    h = pkg.Handle(pkg._lib.make_mrf_config(blk.channels, ks, ds, precision="f16x3",
                                            resblock=blk.resblock), -1, mrf=True)
    sd = block_state(blk)
    for jj, j in enumerate(blk.blocks):
        for pre, _ in block_convs(blk, j):
            tail = pre.split(".", 2)[2]
            for leaf in (".weight", ".bias"):
                h.set_weight(f"resblocks.{jj}.{tail}{leaf}", torch.from_numpy(sd[pre + leaf]))
    st = h.plan()["stages"][0]
    if st["thin"]:
        # the plan lists the thin launch's halos, the library its kernels' windows; the fp32
        # control runs mrf_thin where f16x3 / bf16x3 run mrf_thin_mfma: one geometry or none
        halo = max(st["thin_halo"])
        nwin = pkg.load_library().hfg_debug_thin_window(blk.channels, 0)
        assert nwin > 0 and (not st["thin_mfma"] or
                             pkg.load_library().hfg_debug_thin_window(blk.channels, 1) == nwin)
        return [(nwin - 2 * halo, halo)]
    out = []
    for rb in st["rbs"]:
        assert rb["fused"], f"{blk.name}: not a whole-block launch"
        if rb["split"]:
            hp0, hp1, w0, w1 = rb["parts"]
            out += [(w0, hp0), (w1, hp1)]
        else:
            out.append((rb["W"], rb["halo"]))
    return out


def spike_geometry(windows):
    """(L, {position name: column}): two full windows plus a partial one of the first launch
    (L = 2 W + 37), or past 1000 columns the smallest L with two windows (W + 1); the spike
    (a) mid-window, (b) on the last column of window 0, (c) on the first column of window 1's
    halo — of every launch of the entry."""
    w0 = windows[0][0]
    L = 2 * w0 + 37 if 2 * w0 + 37 <= 1000 else w0 + 1
    pos = {}
    for i, (w, halo) in enumerate(windows):
        assert w < L, "two windows"
        tag = "" if i == 0 else str(i)
        for name, t in (("a", w // 2), ("b", w - 1), ("c", w - halo)):
            if t not in pos.values():
                pos[name + tag] = t
    return L, pos


def spike_input(blk, L, t0, ratio):
    """x f32[2, C, L]: item 0 = 0.5 randn with column t0 (all channels) times `ratio`; item 1 =
    plain 0.5 randn."""
    x = prng.normal(blk.seed, "x", (2, blk.channels, L), 0.5)
    x[0, :, t0] *= np.float32(ratio)
    return x


def outlier_input(blk, L):
    """x f32[1, C, L]: 0.5 randn with channel C // 3 times 2^12 for all t."""
    x = prng.normal(blk.seed, "x", (1, blk.channels, L), 0.5)
    x[0, blk.channels // 3] *= np.float32(OUTLIER_GAIN)
    return x


def exact_max_input(blk, L, k, under):
    """x f32[1, C, L]: |x| <= 0.9 * 2^k except one element, which is exactly 2^k (or, with
    `under`, the float just below it, 2^k (1 - 2^-24))."""
    x = prng.normal(blk.seed, f"x{k}", (1, blk.channels, L), 0.25)
    x = np.clip(x, -0.9, 0.9) * np.float32(2.0 ** k)
    top = np.float32(2.0 ** k)
    x[0, blk.channels // 2, L // 3] = np.nextafter(top, np.float32(0)) if under else top
    assert float(np.abs(x).max()) == float(2.0 ** k) * ((1 - 2.0 ** -24) if under else 1.0)
    return x.astype(np.float32)


@dataclass
class BlockRef:
    ref64: np.ndarray      # float64 [B, C, L]
    ref32: np.ndarray      # the fp32 torch oracle, as float64
    allowance: float       # f16x3 underflow allowance of item 0's chain (see underflow_allowance)
    sens: np.ndarray       # case 2: |w| (*) |x| of the first conv + |x|, float64 [B, C, L]


def underflow_allowance(operands):
    """The documented f16x3 underflow allowance of a conv chain, in float64 from the reference
    operands: sum over the convs of  2 * 2^-39 * max|operand| * max_row sum|w|.

    Derivation (csrc/bf16x3_common.h): an operand is scaled so that its tensor's largest
    magnitude m lands in [2^14, 2^15); an element the scaling leaves under the f16 normal
    range is stored as hi + lo with an absolute error of at most half the subnormal quantum
    2^-24 in the scaled domain, i.e. <= 2^-25 / 2^14 * m = 2^-39 m.  A conv output sums those
    errors weighted by |w| along one weight row: <= 2^-39 m sum|w|.  The weights are split the
    same way against their layer's maximum, which contributes as much again: the factor 2."""
    return float(sum(2.0 * 2.0 ** -39 * float(np.abs(op).max()) * float(np.abs(w).sum((1, 2)).max())
                     for op, w in operands))


def _block_ref(blk, x):
    sd = block_state(blk)
    sd64 = {k: v.astype(np.float64) for k, v in sd.items()}
    x64 = x.astype(np.float64)
    outs, allow, sens = [], 0.0, None
    for j in blk.blocks:
        xr, operands = x64, []
        convs = block_convs(blk, j)
        for i, (pre, d) in enumerate(convs):
            k = blk.kernels[j]
            second = blk.resblock != "2" and i % 2 == 1
            op = N.lrelu(xt if second else xr)
            w = sd64[pre + ".weight"]
            operands.append((op[:1], w))
            if i == 0 and sens is None:
                sens = N.conv1d(np.abs(x64), np.abs(w), np.zeros(w.shape[0]),
                                C.get_padding(k, d), d) + np.abs(x64)
            xt = N.conv1d(op, w, sd64[pre + ".bias"], C.get_padding(k, d), d)
            if blk.resblock == "2" or second:
                xr = xr + xt
        outs.append(xr)
        allow = max(allow, underflow_allowance(operands))
    ref64 = sum(outs) / len(outs)
    tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
    with torch.no_grad():
        o32 = [block_forward(tsd, f"resblocks.{j}", torch.from_numpy(np.array(x)), blk.kernels[j],
                             blk.dilations[j], blk.resblock) for j in blk.blocks]
        r32 = o32[0]
        for o in o32[1:]:
            r32 = r32 + o
        r32 = r32 / len(o32) if len(o32) > 1 else r32
    return BlockRef(ref64, r32.numpy().astype(np.float64), allow, sens)


_BLOCKS = {b.name: b for b in SPIKE_BLOCKS + OUTLIER_BLOCKS + [EXACT_BLOCK, GRID_BLOCK]}


@functools.lru_cache(maxsize=None)
def spike_case(pkg, name, pos, ratio):
    """(x, BlockRef, t0, L) of one spike input; computed once per session and shared."""
    blk = _BLOCKS[name]
    L, positions = spike_geometry(block_windows(pkg, blk))
    x = spike_input(blk, L, positions[pos], ratio)
    x.setflags(write=False)
    return x, _block_ref(blk, x), positions[pos], L


def spike_positions(pkg, name):
    return list(spike_geometry(block_windows(pkg, _BLOCKS[name]))[1])


@functools.lru_cache(maxsize=None)
def outlier_case(pkg, name):
    blk = _BLOCKS[name]
    L = block_windows(pkg, blk)[0][0] + 37
    x = outlier_input(blk, L)
    x.setflags(write=False)
    return x, _block_ref(blk, x)


@functools.lru_cache(maxsize=None)
def exact_max_case(k, under):
    x = exact_max_input(EXACT_BLOCK, 300, k, under)
    x.setflags(write=False)
    return x, _block_ref(EXACT_BLOCK, x)


GRID_SPIKE, GRID_L = 10, 120


@functools.lru_cache(maxsize=None)
def subnormal_grid_case():
    """x f32[1, 64, 120]: column 10 is 1.5 * 2^14 in every channel, so the tensor's scale
    exponent is exactly 0 (15 - frexp exponent 15); every other element is an odd multiple
    (2 n + 1) 2^-24, n < 8: on the f16 subnormal grid at that scale and exactly representable,
    and half-way between two grid points at any smaller scale."""
    n = (prng.uniform01(GRID_BLOCK.seed, "grid", 64 * GRID_L) * 8).astype(np.int64).reshape(1, 64, GRID_L)
    x = ((2 * n + 1) * 2.0 ** -24).astype(np.float32)
    x[0, :, GRID_SPIKE] = np.float32(1.5 * 2.0 ** 14)
    x.setflags(write=False)
    return x, _block_ref(GRID_BLOCK, x)


# ----------------------------------------------------------------------------------------
# bars
# ----------------------------------------------------------------------------------------
def region_masks(L, t0, radius):
    """(hot, quiet) boolean masks over L columns: hot = within `radius` of column t0."""
    t = np.arange(L)
    hot = np.abs(t - t0) <= radius
    return hot, ~hot


def region_check(got, ref64, ref32, mask, rtol, allowance=0.0):
    """(err, bar, cond, scale) of the stage rule restricted to the columns in `mask` (all
    columns with mask None): err = max|got - ref64|, bar = max(rtol * max(1, max|ref64|),
    4 * max|ref32 - ref64|) + allowance."""
    sl = (Ellipsis, slice(None) if mask is None else mask)
    r = ref64[sl]
    with np.errstate(invalid="ignore"):
        err = float(np.abs(np.asarray(got, np.float64)[sl] - r).max())
        cond = float(np.abs(ref32[sl] - r).max())
    scale = float(np.abs(r).max())
    return err, max(rtol * max(1.0, scale), 4 * cond) + allowance, cond, scale


def quiet_reference_ok(ref64, quiet, min_cover=0.6):
    """The quiet region covers at least 60 % of the columns and its reference is finite and
    not identically zero."""
    r = ref64[..., quiet]
    return bool(quiet.mean() >= min_cover and np.isfinite(r).all() and np.abs(r).max() > 0)


# ----------------------------------------------------------------------------------------
# generators
# ----------------------------------------------------------------------------------------
C128X2 = C.GenConfig(upsample_rates=[8, 8], upsample_kernel_sizes=[16, 16],
                     upsample_initial_channel=128)
GEN_CONFIGS = {"v1": C.V1, "v2star": C.V2STAR, "c128x2": C128X2}
LOG_FLOOR = float(np.log(1e-5))   # digital silence of a ln(clamp(mel, 1e-5)) front end


def gen_state(name, seed=131):
    return C.make_state_dict(GEN_CONFIGS[name], seed=seed)


def make_generator(pkg, name, precision, dev, sd=None):
    gen = pkg.HiFiGANGenerator(**GEN_CONFIGS[name].kwargs(), precision=precision).eval()
    gen.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v))
                         for k, v in (sd or gen_state(name)).items()})
    return gen.to(dev)


def rf_frames(cfg):
    """HiFiGANGenerator.receptive_field_frames restated from the config (host-side, no module)."""
    rate, halo = 1, 3.0
    for u, k in zip(cfg.upsample_rates, cfg.upsample_kernel_sizes):
        halo += -(-k // u) / rate
        rate *= u
        halo += max(sum(C.get_padding(kr, d) + C.get_padding(kr, 1) for d in dils)
                    for kr, dils in zip(cfg.resblock_kernel_sizes, cfg.resblock_dilation_sizes)) / rate
    return int(halo + 3.0 / rate) + 1


def stage_rates(cfg):
    """{tap name: columns per mel frame}, "wav" included."""
    rates, r = {"conv_pre": 1}, 1
    for i, u in enumerate(cfg.upsample_rates):
        r *= u
        rates[f"ups.{i}"] = rates[f"mrfs.{i}"] = r
    rates["wav"] = r
    return rates


def _tone_frames(seed, freq):
    """16 log-mel frames [80, 16] (float64, natural log, floored at ln 1e-5) of a seeded
    tone + noise, through oracle/mel_torch.log_mel."""
    from oracle import mel_torch
    n = 15 * mel_torch.CONFIG["hop_length"]
    t = np.arange(n) / mel_torch.CONFIG["sample_rate"]
    wav = 0.3 * np.sin(2 * np.pi * freq * t) + prng.normal(seed, "noise", (n,), 0.01)
    lm = mel_torch.log_mel(torch.from_numpy(wav.astype(np.float32))).numpy().astype(np.float64)
    assert lm.shape == (80, 16)
    return np.maximum(lm * np.log(10.0), LOG_FLOOR)


@functools.lru_cache(maxsize=None)
def logmel_input():
    """mel f32[2, 80, 48], built in float64: item 0 = tone | exact silence (frames 16-31, every
    bin ln 1e-5) | tone, item 1 = silence everywhere."""
    mel = np.full((2, 80, 48), LOG_FLOOR, np.float64)
    mel[0, :, :16] = _tone_frames(141, 440.0)
    mel[0, :, 32:] = _tone_frames(142, 1760.0)
    mel = mel.astype(np.float32)
    mel.setflags(write=False)
    return mel


LOGMEL_QUIET = (20, 28)   # frames of item 0 taken as the quiet region


def gen_refs(name, mel, sd=None):
    """({tap: float64 ref}, {tap: fp32 oracle as float64}) of a generator, "wav" included."""
    cfg, sd = GEN_CONFIGS[name], sd or gen_state(name)
    r64, r32 = {}, {}
    r64["wav"] = N.generator_forward(sd, cfg, mel, tap=lambda n, t: r64.__setitem__(n, t.copy()))
    with np.errstate(all="ignore"):
        H.generator_forward(H.to_torch_state(sd), cfg, torch.from_numpy(np.array(mel)),
                            tap=lambda n, t: r32.__setitem__(n, t.numpy().astype(np.float64)))
    return r64, r32


@functools.lru_cache(maxsize=None)
def logmel_refs(name):
    return gen_refs(name, logmel_input())


EXTREME_LENS = [12, 7, 12, 3]
EXTREME_GAINS = [2.0 ** -40, 1.0, 2.0 ** 40, 0.0]


@functools.lru_cache(maxsize=None)
def extremes_input():
    """mel f32[4, 80, 12]: randn times [2^-40, 1, 2^40, 0], zero past each item's length."""
    mel = prng.normal(151, "mel", (4, 80, 12))
    for b, (g, n) in enumerate(zip(EXTREME_GAINS, EXTREME_LENS)):
        mel[b] *= np.float32(g)
        mel[b, :, n:] = 0
    mel.setflags(write=False)
    return mel


@functools.lru_cache(maxsize=None)
def extremes_refs(name, b):
    """References of item b run alone on its own length."""
    return gen_refs(name, extremes_input()[b:b + 1, :, :EXTREME_LENS[b]])


NAN_FRAME = 20


def nan_input(T, value):
    """mel f32[3, 80, T] randn; item 1 has `value` (NaN / inf) in every bin of frame 20."""
    mel = prng.normal(161, "mel", (3, 80, T))
    mel[1, :, NAN_FRAME] = value
    return mel


@functools.lru_cache(maxsize=None)
def nan_oracle(T, bf16_weights):
    """The fp32 oracle's wav [3, 1, L] of nan_input(T, NaN) (bf16w: on bf16-rounded weights)."""
    sd = H.to_torch_state(gen_state("v1"))
    if bf16_weights:
        sd = {k: (v.to(torch.bfloat16).float() if k.endswith(".weight") else v) for k, v in sd.items()}
    return H.generator_forward(sd, C.V1, torch.from_numpy(nan_input(T, np.nan))).numpy()
