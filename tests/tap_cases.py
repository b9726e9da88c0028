"""Cases, probes, float64 references and mutants of the tap-geometry tests (test_taps_host.py,
test_gpu_taps.py).  Not a test module and not a conftest: plain helpers on top of seam_cases.py.

What is under test: the taps themselves.  The planner and the launchers hold a dozen hard
limits on kernel sizes, dilations and upsampling rates, each a constant that sizes an LDS margin
or a staging register file (LIMITS below).  Every case here sits exactly on one of them, one
step inside it, or on the first configuration past it (which then runs another kernel, or is
refused when the handle is created), on probe weights whose outermost tap is as loud as any
other path: an LDS read one row past a margin returns a neighbour's bytes, not a fault, and
with default-init weights it would carry 1e-5 of the output.

CASES: standalone ResBlock / ResBlock2 / MRF modules (seam_cases' probes, lengths and windows).
UPS_CASES: one-stage generators whose ups.0 reads the mel itself (conv_pre = centre-tap
identity) on weights with every tap loud and distinct.
REFUSALS: one step past each refusing limit; host only, never launched.

Each case pins what the plan must say of it (`pin16`, `pin32`: signature() of the f16x3 and the
fp32 plan) and the quantity it puts on its limit; a retuned constant fails test_taps_host.py
with the name of the case to move.  No tolerance is introduced here: ResBlock / MRF / ups
tensors go under test_gpu_stages.py's stage bar with cond = 0 (the probes are exact), wavs under
the project's 1e-4.
"""
import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

import seam_cases as S
from oracle import config as C
from oracle import hifigan_np64 as N
from oracle import prng
from seam_cases import Block

# The constants the cases touch, as this suite reads them (csrc/kernels.h, csrc/plan.cpp).
# They are restated, not read: the library exports the plan, not its constants, and the plan
# of every case is pinned below, so a retune shows as a plan that no longer matches its case.
LIMITS = {
    "rb_marg(C <= 64, 512)": 48,     # kernels.h rb_marg: spare operand rows of resblock_bf16x3
    "rb_marg(64, 256)": 16,
    "rb_marg(128, 256)": 28,         # not reachable: C = 128 has a k = 3 instance only, d <= 16
    "window floor 512 / 4": 128,     # plan.cpp window_width: W >= nwin / 4
    # plan.cpp plan_resblocks: C = 128, nwin / W <= 1.15 on the 256-column window
    "C = 128 halo cap": max(h for h in range(64) if 256 / ((256 - 2 * h) & ~3) <= 1.15),
    "kRbMaxConv": 16,
    "kMaxDil": 16,                   # kernels.h bf16x3_supported
    "bf16x3 taps": 16,
    "kBf16x3MaxHalo": 128,
    "halo_max(0)": 192,              # the fp32 kernel's runtime-KT instance
    "kThinMarg": 64,
    "thin floor 512 / 4": 128,       # plan.cpp plan_thin: nwin - 2 halo_max >= nwin / 4
}


@dataclass(frozen=True)
class TapCase:
    blk: Block
    launch: str                  # seam_cases.Case.launch: what the split-precision plans run
    why: str                     # the launch it exists for and what sits on the limit
    limit: Optional[Tuple[str, str, str]]   # (quantity(), relation, key of LIMITS)
    pin16: tuple                 # signature() of the f16x3 plan
    pin32: tuple                 # ... of the fp32 plan
    nwin: int = 0                # the window the limit quantity W / thin_W is computed on
    sparse: int = 0              # 0: x in {0 .. 3}; n: x in {0, 1}, one element in n set
    bias_from: int = 0           # convs before this one (execution order) have zero biases
    spike: int = 0               # x = spike on the element that feeds each seam's halo edge
    # the stage bar the bf16x3 run is held to.  One tap path of the 16-conv list is 5^-8 of
    # the output, on at most 32 channels x 147 shifts at best 1 / 83 of its largest value:
    # under 100 bars of 4e-5 whatever the input.  Every value of the probe is an integer
    # < 2^16, exact in bf16 hi + lo, so that case holds bf16x3 to the bar bf16w already
    # borrows, f16x3's (seam_cases.RTOL), under which the same path is 449 bars
    bf16x3_bar: str = "bf16x3"

    def rtol(self, precision):
        return S.RTOL[self.bf16x3_bar if precision == "bf16x3" else precision]

    @property
    def name(self):
        return self.blk.name

    @property
    def fp32_convs(self):
        """Convs (execution order) that run the fp32 kernel inside a split-precision handle."""
        return tuple(i for i, (prec, *_) in enumerate(self.pin16[-1]) if prec == 0)

    @property
    def knob_sets(self):
        """seam_cases.knob_sets; a layer case without a small-tile packing has one set."""
        if self.launch == "layer" and all(small < 0 for *_, small in self.pin16[-1]):
            return [{}]
        return S.knob_sets(self)


def signature(plan):
    """What a case pins of a plan dump: the launch kind with its window geometry, and per conv
    (execution order of the first block) (prec, tile, CK, small tile)."""
    st = plan["stages"][0]
    by_mod = {L["mod"]: (L["prec"], L["tile"], L["CK"], L["small"][0]) for L in plan["layers"]}
    order = [m for m in by_mod if ".convs1." in m or ".convs." in m]
    lay = []
    for m in order:
        lay.append(by_mod[m])
        if ".convs1." in m:
            lay.append(by_mod[m.replace(".convs1.", ".convs2.")])
    lay = tuple(lay[:len(lay) // len(st["rbs"])])
    if st["thin"]:
        return ("thin", st["thin_mfma"], tuple(st["thin_halo"]), lay)
    rb = st["rbs"][0]
    if rb["fused"]:
        return ("rb", rb["kt"], rb["nwin"], rb["halo"], rb["W"], rb["split"],
                tuple(rb.get("parts") or ()), lay)
    return ("layer", lay)


def _one(name, ch, k, dils, seed, rb="1", mrf=False):
    return Block(name, ch, (k,), (tuple(dils),), rb, j=-1 if mrf else 0, seed=seed)


def _lay(n, *row):
    return (tuple(row),) * n


T2, T1, T3, T5, T6 = (1, 2, 16, -1), (1, 1, 16, 4), (1, 3, 16, 4), (1, 5, 16, 4), (1, 6, 16, 4)
FLOOR7 = (16, 16, 16, 16, 11)   # k = 7: halo 3 + 4 * 3 + 3 * 59 = 192, r_max 48
FLOOR11 = (9, 9, 9, 9, 6)       # k = 11: halo 190 (5 | every radius: 192 is not reachable)
THIN_FLOOR = (16, 16, 16, 16, 16, 10)   # k = 5: halo 2 * (96) = 192
# 8 distinct dilations: the 5^8 tap paths of 16 convs scatter over as many shifts as a halo
# <= 192 allows (d = (1,) * 8 stacks them on 33 shifts and no probe resolves one path)
CONVS16 = (16, 13, 11, 9, 7, 5, 3, 1)

CASES = [
    # ---- whole-block margin: every (k - 1) / 2 * d must fit the spare operand rows
    TapCase(_one("rb_c32_k7_d16", 32, 7, (16,), 501), "fused",
            "resblock_bf16x3 C = 32: r = 48 fills the margin", ("r_max", "==", "rb_marg(C <= 64, 512)"),
            ("rb", 7, 512, 3, 504, 0, (), _lay(2, *T2)), ("layer", _lay(2, 0, 2, 4, -1))),
    TapCase(_one("rb_c32_k11_d9", 32, 11, (9,), 502), "fused",
            "k = 11: r = 45, the last dilation inside the margin", ("r_max", "<", "rb_marg(C <= 64, 512)"),
            ("rb", 11, 512, 5, 500, 0, (), _lay(2, *T2)), ("layer", _lay(2, 0, 2, 4, -1))),
    TapCase(_one("rb_c32_k11_d10", 32, 11, (10,), 503), "layer",
            "k = 11: r = 50, the first dilation off the margin: layer launches",
            ("r_max", ">", "rb_marg(C <= 64, 512)"),
            ("layer", _lay(2, *T2)), ("layer", _lay(2, 0, 2, 4, -1))),
    TapCase(_one("rb_c64_k3_d16", 64, 3, (16,), 504), "fused",
            "the 256-column C = 64 window: r = 16 fills its margin", ("r_max", "==", "rb_marg(64, 256)"),
            ("rb", 3, 256, 1, 252, 0, (), _lay(2, *T1)), ("layer", _lay(2, 0, 1, 8, -1))),
    # ---- C = 128 recompute cap (the halo does not count the first conv's radius)
    TapCase(_one("rb_c128_k3_cap", 128, 3, (1, 3, 10), 505), "fused",
            "C = 128: halo 16, W 224, nwin / W = 1.143", ("halo", "==", "C = 128 halo cap"),
            ("rb", 3, 256, 16, 224, 0, (), _lay(6, *T5)), ("layer", _lay(6, 0, 0, 8, -1))),
    TapCase(_one("rb_c128_k3_over", 128, 3, (1, 4, 10), 506), "layer",
            "C = 128: halo 17, W 220, nwin / W = 1.164: layer launches on the AREG tile",
            ("halo", ">", "C = 128 halo cap"),
            ("layer", _lay(6, *T5)), ("layer", _lay(6, 0, 0, 8, -1))),
    # ---- window floor W >= nwin / 4
    TapCase(_one("rb_c32_k7_floor", 32, 7, FLOOR7, 507), "split",
            "halo 192: W = 128 = nwin / 4 exactly, with r = 48 on the margin",
            ("W", "==", "window floor 512 / 4"),
            ("rb", 7, 512, 192, 128, 4, (54, 90, 404, 332), _lay(10, *T2)),
            ("layer", _lay(10, 0, 2, 4, -1)), nwin=512, spike=256),
    TapCase(_one("rb_c64_k7_floor", 64, 7, FLOOR7, 508), "split",
            "the same on the C = 64 (persistent) instances", ("W", "==", "window floor 512 / 4"),
            ("rb", 7, 512, 192, 128, 4, (54, 90, 404, 332), _lay(10, *T1)),
            ("layer", _lay(10, 0, 1, 4, -1)), nwin=512, spike=256),
    TapCase(_one("rb_c32_k7_floor_off", 32, 7, FLOOR7[:4] + (12,), 509), "layer",
            "halo 195: W = 120 < 128, layer launches", ("W", "<", "window floor 512 / 4"),
            ("layer", _lay(10, *T2)), ("layer", _lay(10, 0, 2, 4, -1)), nwin=512),
    TapCase(_one("rb_c32_k11_floor", 32, 11, FLOOR11, 510), "split",
            "k = 11: halo 190, W = 132, the last window above the floor",
            ("W", ">", "window floor 512 / 4"),
            ("rb", 11, 512, 190, 132, 4, (55, 90, 400, 332), _lay(10, *T2)),
            ("layer", _lay(10, 0, 2, 4, -1)), nwin=512, spike=256),
    TapCase(_one("rb_c32_k11_floor_off", 32, 11, FLOOR11[:4] + (7,), 511), "layer",
            "k = 11: halo 195, W = 120", ("W", "<", "window floor 512 / 4"),
            ("layer", _lay(10, *T2)), ("layer", _lay(10, 0, 2, 4, -1)), nwin=512),
    # ---- conv count
    TapCase(_one("rb_c32_k7_16convs", 32, 7, CONVS16, 512), "split",
            "8 dilations: 16 convs in one packed stream, split 6 + 10, with r = 48 on the margin",
            ("n_conv", "==", "kRbMaxConv"),
            ("rb", 7, 512, 171, 168, 6, (81, 63, 348, 384), _lay(16, *T2)),
            ("layer", _lay(16, 0, 2, 4, -1)), sparse=4096, bias_from=12, spike=32,
            bf16x3_bar="f16x3"),
    # ---- a split point off V1's
    TapCase(_one("rb_c64_k7_d1357", 64, 7, (1, 3, 5, 7), 513), "split",
            "four pairs: split after the second, halos 15 / 27, W 480 / 456", None,
            ("rb", 7, 512, 57, 396, 4, (15, 27, 480, 456), _lay(8, *T1)),
            ("layer", _lay(8, 0, 1, 4, -1))),
    # ---- ResBlock2 margin
    TapCase(_one("rb2_c32_k7_d16", 32, 7, (16,), 514, "2"), "rb2",
            "resblock2_bf16x3: one conv, r = 48, no halo", ("r_max", "==", "rb_marg(C <= 64, 512)"),
            ("rb", 7, 512, 0, 512, 0, (), _lay(1, *T2)), ("layer", _lay(1, 0, 2, 4, -1))),
    TapCase(_one("rb2_c32_k7_d1_16", 32, 7, (1, 16), 515, "2"), "rb2",
            "resblock2_bf16x3: r = 48 on the second conv: halo 48",
            ("r_max", "==", "rb_marg(C <= 64, 512)"),
            ("rb", 7, 512, 48, 416, 0, (), _lay(2, *T2)), ("layer", _lay(2, 0, 2, 4, -1))),
    # ---- split-precision layer kernel
    TapCase(_one("layer_c256_k9_d16", 256, 9, (16,), 516), "layer",
            "(kt - 1) d = 128 at d = 16 on the runtime-KT instance of tile 3",
            ("span", "==", "kBf16x3MaxHalo"),
            ("layer", _lay(2, *T3)), ("layer", _lay(2, 0, 0, 4, -1))),
    TapCase(_one("layer_c256_k11_d12", 256, 11, (12,), 517), "layer",
            "AREG at its largest reach: (kt - 1) d = 120", ("span", "<", "kBf16x3MaxHalo"),
            ("layer", _lay(2, *T6)), ("layer", _lay(2, 0, 0, 4, -1))),
    TapCase(_one("layer_c256_k5_d16", 256, 5, (16,), 518), "layer",
            "d = 16 on a compile-time AREG instance", ("dil", "==", "kMaxDil"),
            ("layer", _lay(2, *T6)), ("layer", _lay(2, 0, 0, 8, -1))),
    TapCase(_one("layer_c128_k1", 128, 1, (1,), 519), "layer",
            "KT = 1 on the runtime-KT instance", ("kt", "<", "bf16x3 taps"),
            ("layer", _lay(2, *T3)), ("layer", _lay(2, 0, 0, 4, -1))),
    TapCase(_one("layer_c128_k13_d10", 128, 13, (10,), 520), "layer",
            "KT = 13, (kt - 1) d = 120", ("kt", "<", "bf16x3 taps"),
            ("layer", _lay(2, *T3)), ("layer", _lay(2, 0, 0, 4, -1))),
    TapCase(_one("layer_c128_k15_d9", 128, 15, (9,), 521), "layer",
            "KT = 15, the last odd tap count of the split kernel, (kt - 1) d = 126",
            ("span", "<", "kBf16x3MaxHalo"),
            ("layer", _lay(2, *T3)), ("layer", _lay(2, 0, 0, 4, -1))),
    # ---- the fp32 layer kernel inside a split-precision handle
    TapCase(_one("f32in_c128_k11_d13", 128, 11, (13,), 522), "layer",
            "(kt - 1) d = 130 > 128: conv1 on conv1d_mfma_f32, conv2 split again and reading the "
            "scale slot the fp32 kernel published", ("span", ">", "kBf16x3MaxHalo"),
            ("layer", ((0, 0, 4, -1), T5)), ("layer", _lay(2, 0, 0, 4, -1))),
    TapCase(_one("f32in_c128_k17_d1", 128, 17, (1,), 523), "layer",
            "KT = 17 > 16: both convs on the fp32 kernel", ("kt", ">", "bf16x3 taps"),
            ("layer", _lay(2, 0, 0, 4, -1)), ("layer", _lay(2, 0, 0, 4, -1))),
    TapCase(_one("f32in_c128_k17_d12", 128, 17, (12,), 524), "layer",
            "KT = 17 at (kt - 1) d = 192, the fp32 runtime-KT instance's whole staging window",
            ("span", "==", "halo_max(0)"),
            ("layer", _lay(2, 0, 0, 4, -1)), ("layer", _lay(2, 0, 0, 4, -1))),
    TapCase(_one("f32_c64_k13_d16", 64, 13, (16,), 525), "layer",
            "(kt - 1) d = 192 on the 256-column fp32 tile; conv2 split", ("span", "==", "halo_max(0)"),
            ("layer", ((0, 1, 4, -1), T1)), ("layer", _lay(2, 0, 1, 4, -1))),
    # ---- thin whole-MRF kernels
    TapCase(_one("thin_c8_k11_d12", 8, 11, (12,), 526, mrf=True), "thin",
            "mrf_thin C = 8: r = 60, the last k = 11 dilation inside the margin",
            ("r_max", "<", "kThinMarg"),
            ("thin", 0, (65,), _lay(2, 0, 2, 4, -1)), ("thin", 0, (65,), _lay(2, 0, 2, 4, -1))),
    TapCase(_one("thin_c16_k11_d12", 16, 11, (12,), 527, mrf=True), "thin",
            "mrf_thin C = 16 (k = 11 has no MFMA variant): r = 60", ("r_max", "<", "kThinMarg"),
            ("thin", 0, (65,), _lay(2, 0, 2, 4, -1)), ("thin", 0, (65,), _lay(2, 0, 2, 4, -1))),
    TapCase(_one("thin_c8_k9_d16", 8, 9, (16,), 528, mrf=True), "thin",
            "mrf_thin C = 8: r = 64 fills the margin", ("r_max", "==", "kThinMarg"),
            ("thin", 0, (68,), _lay(2, 0, 2, 4, -1)), ("thin", 0, (68,), _lay(2, 0, 2, 4, -1))),
    TapCase(_one("thin_c16_k9_d16", 16, 9, (16,), 529, mrf=True), "thin",
            "mrf_thin C = 16: r = 64 fills the margin", ("r_max", "==", "kThinMarg"),
            ("thin", 0, (68,), _lay(2, 0, 2, 4, -1)), ("thin", 0, (68,), _lay(2, 0, 2, 4, -1))),
    TapCase(_one("thinoff_c8_k11_d13", 8, 11, (13,), 530, mrf=True), "layer",
            "r = 65: not thin; C = 8 has no split tile: fp32 layer launches in every precision",
            ("r_max", ">", "kThinMarg"),
            ("layer", _lay(2, 0, 2, 4, -1)), ("layer", _lay(2, 0, 2, 4, -1))),
    TapCase(_one("thinoff_c16_k11_d13", 16, 11, (13,), 531, mrf=True), "layer",
            "the same at C = 16", ("r_max", ">", "kThinMarg"),
            ("layer", _lay(2, 0, 2, 4, -1)), ("layer", _lay(2, 0, 2, 4, -1))),
    TapCase(_one("thin_c16_floor", 16, 5, THIN_FLOOR, 532, mrf=True), "thin_mfma",
            "halo 192: nwin - 2 halo = 128 = nwin / 4 on both thin kernels",
            ("thin_W", "==", "thin floor 512 / 4"),
            ("thin", 1, (192,), _lay(12, 0, 2, 8, -1)), ("thin", 0, (192,), _lay(12, 0, 2, 8, -1)),
            nwin=512, sparse=64, bias_from=8, spike=256),
    TapCase(_one("thin_c16_floor_off", 16, 5, THIN_FLOOR[:5] + (11,), 533, mrf=True), "layer",
            "halo 194: 4 columns short of the floor, fp32 layer launches",
            ("thin_W", "<", "thin floor 512 / 4"),
            ("layer", _lay(12, 0, 2, 8, -1)), ("layer", _lay(12, 0, 2, 8, -1)),
            nwin=512, sparse=64, bias_from=8),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def all_convs(blk):
    return [c for j in blk.blocks for c in S.case_convs(blk, j)]


def quantity(case, what):
    """The quantity a case puts on its limit, from its lists alone."""
    convs = all_convs(case.blk)
    rad = [S.radius(k, d) for _, k, d, _ in convs]
    k, dmax = case.blk.kernels[0], max(d for _, _, d, _ in convs)
    halo = sum(rad) - rad[0]
    return {"r_max": max(rad), "halo": halo, "thin_halo": sum(rad), "n_conv": len(convs),
            "span": (k - 1) * dmax, "dil": dmax, "kt": k,
            "W": (case.nwin - 2 * halo) & ~3, "thin_W": case.nwin - 2 * sum(rad)}[what]


# one step past each refusing limit: (name, factory of the config, module the message names,
# the span or sizes it names)
def _mrf_refusal(ch, k, dils):
    return lambda pkg, precision: pkg._lib.make_mrf_config(ch, [k], [list(dils)], precision=precision)


def _gen_refusal(u, k):
    cfg = C.GenConfig(upsample_rates=[u], upsample_kernel_sizes=[k], upsample_initial_channel=64,
                      resblock_kernel_sizes=[3], resblock_dilation_sizes=[[1]])
    return lambda pkg, precision: pkg.make_config(**cfg.kwargs(), precision=precision)


REFUSALS = [
    # fp32 specialised k = 3 stages (3 - 1) * 16 = 32 columns
    ("c64_k3_d17", _mrf_refusal(64, 3, (17,)), True, "resblocks.0.convs1.0", ("34", "32")),
    ("c32_k7_d17", _mrf_refusal(32, 7, (17,)), True, "resblocks.0.convs1.0", ("102", "96")),
    ("c256_k11_d17", _mrf_refusal(256, 11, (17,)), True, "resblocks.0.convs1.0", ("170", "160")),
    # the runtime-KT instance: 192
    ("c64_k13_d17", _mrf_refusal(64, 13, (17,)), True, "resblocks.0.convs1.0", ("204", "192")),
    ("c128_k17_d13", _mrf_refusal(128, 17, (13,)), True, "resblocks.0.convs1.0", ("208", "192")),
    # 9 dilations: one past HFG_MAX_DIL = 8, i.e. 18 convs against kRbMaxConv = 16 (refused when
    # the configuration is built, before there is a handle)
    ("c32_k3_9dil", _mrf_refusal(32, 3, (1,) * 9), True, "ResBlock", ("too many dilations",)),
    # k < u upsamplers
    ("ups_u4_k3", _gen_refusal(4, 3), False, "ups.0", ("kernel 3", "stride 4")),
    ("ups_u8_k7", _gen_refusal(8, 7), False, "ups.0", ("kernel 7", "stride 8")),
    ("ups_u2_k1", _gen_refusal(2, 1), False, "ups.0", ("kernel 1", "stride 2")),
]


# ----------------------------------------------------------------------------------------
# probe weights, inputs and float64 references of the ResBlock / MRF cases
# ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tap_state(name):
    """seam_cases.probe_state of the case; the long lists with the biases of their first
    `bias_from` convs zeroed (a bias of 1 ahead of p pairs arrives as 5^p)."""
    case = BY_NAME[name]
    sd = S.probe_state(case.blk)
    if not case.bias_from:
        return sd
    sd = {k: np.array(v) for k, v in sd.items()}
    for pre, *_ in all_convs(case.blk)[:case.bias_from]:
        sd[pre + ".bias"][:] = 0.0
    for v in sd.values():
        v.setflags(write=False)
    return sd


def edge_feeds(pkg, blk):
    """[(column, key)] of x: the columns a launch window one column short of its halo would
    miss, at its first two seams on either side.  A thin window holds x itself on
    [s - halo, s + W + halo); a whole-block window holds its first conv's output there, which
    that conv reads r0 further out."""
    out = []
    for w in S.block_windows(pkg, blk):
        if not w.windowed or w.conv0:
            continue
        r0 = S.radius(*S.case_convs(blk, max(w.j, 0))[0][1:3]) if w.first_exact else 0
        for s in (w.W, 2 * w.W):
            out += [(s - w.halo - r0, f"{w.tag}{s}l"), (s + w.halo - 1 + r0, f"{w.tag}{s}r")]
    return out


@functools.lru_cache(maxsize=None)
def tap_input(pkg, name, L, B=2):
    """x f32 [B, C, L]: seam_cases.probe_input, or for a `sparse` case zeros and ones; a `spike`
    case has that value on one seeded (item, channel) of every edge_feeds column: in a long
    list one tap path is 5^-pairs of the output, and the path through the halo's last column
    has to carry more than its share to stay above the bars."""
    case = BY_NAME[name]
    blk = case.blk
    if not case.sparse:
        x = S.probe_input(blk.seed, blk.channels, L, B)
    else:
        u = prng.uniform01(blk.seed, f"s{B}x{L}", B * blk.channels * L)
        x = (u * case.sparse < 1.0).astype(np.float32).reshape(B, blk.channels, L)
    if case.spike:
        x = np.array(x)
        for col, key in edge_feeds(pkg, blk):
            if 0 <= col < L:
                u = prng.uniform01(blk.seed, "spike" + key, 2)
                x[int(u[0] * B) % B, int(u[1] * blk.channels) % blk.channels, col] = case.spike
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def tap_ref(pkg, name, L, B=2):
    """(x, float64 reference) of a case at length L; computed once per session and shared."""
    x = tap_input(pkg, name, L, B)
    ref = S.reference(BY_NAME[name].blk, x, tap_state(name))
    ref.setflags(write=False)
    return x, ref


def _conv_outer_moved(f, pre, x, k, d):
    """The conv with its outermost tap k - 1 placed as at dilation d - 1: max(k - 1, 1) columns
    nearer (k = 1: the one tap reads its left neighbour)."""
    w = np.asarray(f[pre + ".weight"], np.float64)
    b = np.asarray(f[pre + ".bias"], np.float64)
    pad = C.get_padding(k, d)
    w0 = w.copy()
    w0[:, :, k - 1] = 0.0
    y = N.conv1d(x, w0, b, pad, d)
    L = x.shape[-1]
    t = np.arange(L) + (k - 1) * d - pad - max(k - 1, 1)
    ok = (t >= 0) & (t < L)
    xs = np.zeros_like(x)
    xs[..., ok] = x[..., t[ok]]
    return y + np.einsum("oc,bcl->bol", w[:, :, k - 1], xs)


def forward64(name, x, moved=None):
    """(output, every intermediate tensor) of the case's module in float64, written out conv by
    conv (oracle/hifigan_np64.py's steps); moved = i: conv i of the first block runs
    _conv_outer_moved."""
    case = BY_NAME[name]
    blk, f = case.blk, tap_state(name)
    outs, seen = [], []
    for n, j in enumerate(blk.blocks):
        xr, xt = np.asarray(x, np.float64), None
        for i, (pre, k, d, second) in enumerate(S.case_convs(blk, j)):
            src = N.lrelu(xt if second else xr)
            if moved == i and n == 0:
                y = _conv_outer_moved(f, pre, src, k, d)
            else:
                y = N.conv1d(src, np.asarray(f[pre + ".weight"], np.float64),
                             np.asarray(f[pre + ".bias"], np.float64), C.get_padding(k, d), d)
            seen.append(y)
            if second or blk.resblock == "2":
                xr = xr + y
                seen.append(xr)
            else:
                xt = y
        outs.append(xr)
    return (sum(outs) / len(outs) if blk.j < 0 else outs[0]), seen


def widest_conv(blk):
    """Index (execution order, first block) of the conv with the largest radius."""
    rad = [S.radius(k, d) for _, k, d, _ in S.case_convs(blk, blk.blocks[0])]
    return int(np.argmax(rad))


# ----------------------------------------------------------------------------------------
# upsampler cases: one-stage generators, ups.0 reads the mel itself
# ----------------------------------------------------------------------------------------
UPS_LIMITS = {"polyphase taps": 16}   # taps per phase of the split kernel's runtime-KT instance
UPS_SEED = 551
UPS_POST_TAPS = S.POST_TAPS


@dataclass(frozen=True)
class UpsCase:
    u: int
    k: int
    c0: int        # n_mels = upsample_initial_channel: ups.0 is c0 -> c0 / 2 channels
    why: str
    pin16: tuple   # ups_signature() of the f16x3 plan: (prec, tile, CK, small tile, frames)
    pin32: tuple
    signed: bool = False   # the mel in {-3 .. 3}: leaky_relu is no identity (0.1f against 0.1)

    @property
    def name(self):
        return f"u{self.u}_k{self.k}" + ("_signed" if self.signed else "")

    @property
    def KT(self):
        return -(-self.k // self.u)

    @property
    def p(self):
        return (self.k - self.u) // 2

    @property
    def limit(self):
        rel = "==" if self.KT == 16 else "<" if self.KT < 16 else ">"
        return ("KT", rel, "polyphase taps")

    @property
    def store(self):
        """The polyphase epilogue's store class (conv_bf16x3.hip: vec4)."""
        return "float4" if self.u % 4 == 0 and self.p % 4 == 0 else "scalar"

    def store_paths(self, L):
        """The epilogue paths a launch on L frames takes, per 32-column tile of its N columns as
        the kernel decides it: "float4" where the whole tile lands inside [0, L_out), "masked
        float4" on the tiles that cross either end, "scalar" where u, p or L_out is no multiple
        of 4.  (The rows of every case here are whole 32-row tiles.)"""
        Lo, N_ = self.out_len(L), self.columns(L)
        if self.store == "scalar" or Lo % 4:
            return {"scalar"}
        inside = lambda nt: (nt + 31 < N_ and nt * self.u - self.p >= 0 and
                             (nt + 32) * self.u - 1 - self.p < Lo)
        return {"float4" if inside(nt) else "masked float4" for nt in range(0, N_, 32)}

    @property
    def frames(self):
        """The plan packs the output-frame kernel (k = 2u, ups_rate_ok, whole row tiles)."""
        return self.pin16[4][0] >= 0

    @property
    def cfg(self):
        return C.GenConfig(n_mels=self.c0, upsample_rates=[self.u], upsample_kernel_sizes=[self.k],
                           upsample_initial_channel=self.c0, resblock_kernel_sizes=[3],
                           resblock_dilation_sizes=[[1]])

    def out_len(self, L):
        return (L - 1) * self.u - 2 * self.p + self.k

    def columns(self, L):
        """GEMM columns of the polyphase launch (forward.cpp run_ups)."""
        return (self.out_len(L) - 1 + self.p) // self.u + 1


def _u(u, k, c0, why, pin16, pin32, **kw):
    return UpsCase(u, k, c0, why, pin16, pin32, **kw)


UPS_CASES = [
    # ---- k = 2u: both kernels; float4 and scalar polyphase stores; the three ups_rate_ok classes
    _u(8, 16, 16, "k = 2u, u % 8 == 0: frames cfg 1; polyphase float4 stores (p = 4)",
       (1, 1, 16, 4, (1, 1)), (0, 1, 16, -1, (-1, 0))),
    _u(8, 16, 16, "the same on a signed mel", (1, 1, 16, 4, (1, 1)), (0, 1, 16, -1, (-1, 0)),
       signed=True),
    _u(4, 8, 32, "k = 2u, u = 4: frames cfg 1; scalar stores (p = 2)",
       (1, 1, 16, 4, (1, 1)), (0, 1, 16, -1, (-1, 0))),
    _u(2, 4, 64, "k = 2u, u = 2: frames cfg 1 (the pair path); scalar stores",
       (1, 1, 16, 4, (1, 1)), (0, 1, 16, -1, (-1, 0))),
    _u(16, 32, 16, "k = 2u, u = 16: frames cfg 0; float4 stores (p = 8)",
       (1, 3, 16, 4, (0, 1)), (0, 0, 16, -1, (-1, 0))),
    # ---- KT = 1, p = 0
    _u(8, 8, 16, "KT = 1, p = 0, float4 stores", (1, 1, 16, 4, (-1, 0)), (0, 1, 4, -1, (-1, 0))),
    _u(4, 4, 16, "KT = 1, p = 0 on the 32-row tile", (1, 2, 16, -1, (-1, 0)), (0, 2, 4, -1, (-1, 0))),
    # ---- KT = 3 on the runtime-KT instance and the float4 path
    _u(4, 12, 16, "KT = 3 generic with float4 stores (p = 4)",
       (1, 2, 16, -1, (-1, 0)), (0, 2, 8, -1, (-1, 0))),
    # ---- k - u odd: L_out = u L + 1, phases one tap short, scalar stores
    _u(4, 9, 16, "k - u odd, p = 2, KT = 3", (1, 2, 16, -1, (-1, 0)), (0, 2, 8, -1, (-1, 0))),
    _u(4, 7, 16, "k - u odd, p = 1, KT = 2", (1, 2, 16, -1, (-1, 0)), (0, 2, 8, -1, (-1, 0))),
    _u(2, 5, 32, "k - u odd, p = 1, KT = 3", (1, 2, 16, -1, (-1, 0)), (0, 2, 8, -1, (-1, 0))),
    _u(2, 3, 32, "k - u odd, p = 0, KT = 2", (1, 2, 16, -1, (-1, 0)), (0, 2, 8, -1, (-1, 0))),
    # ---- u no power of two: the division of row -> (channel, phase); rows off the 32-row grid
    _u(3, 6, 24, "u = 3: 36 rows", (1, 2, 16, -1, (-1, 0)), (0, 2, 8, -1, (-1, 0))),
    _u(3, 7, 24, "u = 3, k - u even, KT = 3", (1, 2, 16, -1, (-1, 0)), (0, 2, 8, -1, (-1, 0))),
    _u(5, 10, 24, "u = 5: 60 rows", (1, 2, 16, -1, (-1, 0)), (0, 2, 8, -1, (-1, 0))),
    _u(5, 5, 24, "u = 5, KT = 1", (1, 2, 16, -1, (-1, 0)), (0, 2, 4, -1, (-1, 0))),
    # ---- stride 1
    _u(1, 3, 64, "stride 1, KT = 3", (1, 2, 16, -1, (-1, 0)), (0, 2, 8, -1, (-1, 0))),
    _u(1, 1, 64, "stride 1, KT = 1", (1, 2, 16, -1, (-1, 0)), (0, 2, 4, -1, (-1, 0))),
    # ---- the runtime-KT instance's last tap count, and the first past it
    _u(2, 32, 32, "KT = 16", (1, 2, 16, -1, (-1, 0)), (0, 2, 4, -1, (-1, 0))),
    _u(2, 34, 32, "KT = 17: the fp32 upsampler inside a split-precision handle",
       (0, 2, 4, -1, (-1, 0)), (0, 2, 4, -1, (-1, 0))),
]
UPS_BY_NAME = {c.name: c for c in UPS_CASES}
assert len(UPS_BY_NAME) == len(UPS_CASES)


def ups_signature(plan):
    L = next(L for L in plan["layers"] if L["mod"] == "ups.0")
    return (L["prec"], L["tile"], L["CK"], L["small"][0], tuple(L["frames"][:2]))


@functools.lru_cache(maxsize=None)
def ups_mel(name, L, B=2):
    """mel f32 [B, c0, L], integers in {0 .. 3} (signed: {-3 .. 3})."""
    case = UPS_BY_NAME[name]
    n = B * case.c0 * L
    m = np.minimum(np.floor(prng.uniform01(UPS_SEED, f"{name}#m{B}x{L}", n) * 4), 3)
    if case.signed:
        m = m * np.where(prng.uniform01(UPS_SEED, f"{name}#s{B}x{L}", n) < 0.5, -1.0, 1.0)
    m = m.astype(np.float32).reshape(B, case.c0, L)
    m.setflags(write=False)
    return m


def ups_weight(case):
    """(weight [C_in, C_out, k], bias [C_out]): every tap loud and distinct,
    weight[(pi(co) + j) % C_in, co, j] = 1 + j % 7; bias in {0, 1}.  (j + 1 up to k = 7; in a
    34-tap kernel a tap of weight 1 among taps up to 34 falls under 100 bf16x3 bars.  No rate
    here is a multiple of 7, so the taps of one phase, j, j + u, ..., differ from their
    neighbours, and 7 in a row are distinct.  Taps j and j' of one output channel share their
    input channel where C_in | j - j' and their weight where 7 | j - j': both only 7 C_in >= 112
    taps apart, past every kernel here, so no (channel, weight) pair occurs twice.)"""
    cin, cout = case.c0, case.c0 // 2
    pi = np.argsort(prng.uniform01(UPS_SEED, case.name + "#pi", cin))[:cout]
    w = np.zeros((cin, cout, case.k), np.float32)
    for j in range(case.k):
        w[(pi + j) % cin, np.arange(cout), j] = 1.0 + j % 7
    b = (prng.uniform01(UPS_SEED, case.name + "#b", cout) < 0.5).astype(np.float32)
    return w, b


@functools.lru_cache(maxsize=None)
def ups_state(name):
    """conv_pre = the centre-tap identity (the stage input is the mel exactly), ups.0 =
    ups_weight, the MRF's one ResBlock on seam_cases' probe weights, conv_post a signed
    power-of-two pattern at the scale that keeps |pre-tanh| <= 1 on an 8-frame mel (a stage value depends on 2 KT
    frames at most; test_taps_host.py asserts |wav| < 0.8 at the case's lengths)."""
    case = UPS_BY_NAME[name]
    cfg = case.cfg
    sd = {k: np.zeros_like(v) for k, v in C.make_state_dict(cfg, seed=UPS_SEED).items()}
    sd["conv_pre.weight"][np.arange(case.c0), np.arange(case.c0), 3] = 1.0
    sd["ups.0.weight"], sd["ups.0.bias"] = ups_weight(case)
    for conv in ("convs1.0", "convs2.0"):
        key = f"mrfs.0.resblocks.0.{conv}"
        sd[key + ".weight"], sd[key + ".bias"] = S.shift_conv(UPS_SEED, name + key, case.c0 // 2, 3)
    box = {}
    N.generator_forward(sd, cfg, ups_mel(name, 8), tap=lambda n, t: box.__setitem__(n, t))
    top = float(np.abs(N.lrelu(box["mrfs.0"])).max()) * sum(abs(s) for *_, s in UPS_POST_TAPS)
    scale = 2.0 ** -int(np.ceil(np.log2(top)))
    for ch, tap, sgn in UPS_POST_TAPS:
        sd["conv_post.weight"][0, ch, tap] = np.float32(sgn * scale)
    for v in sd.values():
        v.setflags(write=False)
    return sd


def ups_tiles(pkg, name):
    """{tag: NTILE} of every kernel tile that can run the case's ups.0, from the f16x3 and the
    fp32 plan: the split tile, the 64-column small tile, the fp32 tile, and the 256-frame tile
    of the output-frame kernel (whose columns are input frames)."""
    p16, p32 = ups_host_plan(pkg, name, "f16x3"), ups_host_plan(pkg, name, "fp32")
    prec, tile, _, small, frames = ups_signature(p16)
    out = {}
    if prec == 1:
        out["tile"] = 32 * S.BF16X3_TILES[tile][4] * S.BF16X3_TILES[tile][2]
        if small >= 0:
            out["small"] = 32 * S.BF16X3_TILES[small][4] * S.BF16X3_TILES[small][2]
    else:
        out["fp32in"] = S.FP32_NTILE[tile]
    out["fp32"] = S.FP32_NTILE[ups_signature(p32)[1]]
    if frames[0] >= 0:
        out["frames"] = 256
    return out


@functools.lru_cache(maxsize=None)
def ups_host_plan(pkg, name, precision="f16x3"):
    case = UPS_BY_NAME[name]
    h = pkg.Handle(pkg.make_config(**case.cfg.kwargs(), precision=precision), -1)
    for k, v in ups_state(name).items():
        h.set_weight(k, torch.from_numpy(np.array(v)))
    h.commit()
    return h.plan()


UPS_MAX_FRAMES = 520


def ups_edges(pkg, name):
    """{L_in: what} that put the launch's column count on a tile edge: polyphase columns
    N = NTILE, output-frame columns L_in = 256."""
    case = UPS_BY_NAME[name]
    out = {}
    for tag, nt in ups_tiles(pkg, name).items():
        for L in range(1, UPS_MAX_FRAMES + 1):
            if (L if tag == "frames" else case.columns(L)) == nt:
                out.setdefault(L, f"{tag} {nt}")
    return out


def ups_lengths(pkg, name):
    """L_in in {1 .. 5} and one column short of, on and past every tile edge."""
    Ls = {1, 2, 3, 4, 5}
    for e in ups_edges(pkg, name):
        Ls |= {e - 1, e, e + 1}
    return sorted(L for L in Ls if 1 <= L <= UPS_MAX_FRAMES)


def ups_ragged_batches(pkg, name):
    """[(T, lens)]: item ends at each position of a frame quad (T = 8), and on both sides of
    every tile edge inside a batch whose width is a multiple of 4 (the output-frame kernel
    runs such batches only)."""
    out = [(8, [8, 7, 6, 5])]
    for e in ups_edges(pkg, name):
        T = (e + 2 + 3) & ~3
        if e >= 8 and T <= UPS_MAX_FRAMES:
            out.append((T, [T, e + 1, e, e - 1]))
    return out


@functools.lru_cache(maxsize=None)
def ups_refs(name, L, B=2, b=None, n=None):
    """{tap: float64} of the case's generator on ups_mel(name, L, B), "wav" included; with
    b / n: of item b alone on its first n frames.  Every weight is bf16-exact (small integers
    and a power of two; test_taps_host.py), so bf16w computes this same model."""
    case = UPS_BY_NAME[name]
    m = np.array(ups_mel(name, L, B))
    if b is not None:
        m = m[b:b + 1, :, :n]
    r = {}
    r["wav"] = N.generator_forward(ups_state(name), case.cfg, m,
                                   tap=lambda k, t: r.__setitem__(k, t.copy()))
    return r


def ups_mutants(name, L, B=2):
    """{mutant: float64 ups.0 tensor} on the float64 restatement alone: the last tap dropped; tap
    0 stored one sample late (the neighbouring phase); the polyphase launch one column short
    (outputs from column N - 1 on never written); the padding off by one."""
    case = UPS_BY_NAME[name]
    sd = ups_state(name)
    x = N.lrelu(np.asarray(ups_mel(name, L, B), np.float64))
    w = np.asarray(sd["ups.0.weight"], np.float64)
    b = np.asarray(sd["ups.0.bias"], np.float64)
    u, k, p = case.u, case.k, case.p
    ref = N.conv_transpose1d(x, w, b, u, p)
    Lo = ref.shape[-1]
    out = {}
    w1 = w.copy()
    w1[:, :, k - 1] = 0.0
    out["last tap dropped"] = N.conv_transpose1d(x, w1, b, u, p)
    w2 = np.concatenate([w, np.zeros_like(w[:, :, :1])], axis=2)
    w2[:, :, 1] += w2[:, :, 0]
    w2[:, :, 0] = 0.0
    out["tap 0 in the next phase"] = N.conv_transpose1d(x, w2, b, u, p)[..., :Lo]
    short = ref.copy()
    short[..., max((case.columns(L) - 1) * u - p, 0):] = 0.0
    out["N one column short"] = short
    moved = np.zeros_like(ref)
    moved[..., :Lo - 1] = ref[..., 1:]
    out["p off by one"] = moved
    return ref, out
