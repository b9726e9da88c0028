"""Probes, window geometry, length classes, float64 references and windowed mutants of the seam
tests (test_seams_host.py, test_gpu_seams.py).  Not a test module and not a conftest: plain
helpers.

What is under test: the time axis of the windowed launches.  resblock_bf16x3 / resblock2_bf16x3
(whole and split), mrf_thin / mrf_thin_mfma and the fused conv_post launch compute a window of
nwin columns and keep its centre W = (nwin - 2 halo) & ~3 (plan.cpp window_width; the thin
kernels W = nwin - 2 halo); a column near a seam is right only if the halo is the summed tap
reach of the later convs and every intermediate is zero outside [0, len).  With default-init
weights the outermost reach carries 1e-5 .. 4e-4 of the output, under the suite's bars
(test_seams_host.py records the figures).  The PROBE weights make that reach as loud as any
other path:

    every conv: weight[co, pi(co), 0] = 1, weight[co, (pi(co) + 1) % C, k - 1] = 1, pi a seeded
    permutation; bias in {0, 1}; x integers in {0 .. 3}

so every activation is a non-negative integer (leaky_relu is the identity), < 2^16: exact in
float64, in fp32 sums and in both split formats (bf16 hi + lo, scaled f16 hi + lo).  The only
inexact step of a probe is the MRF's division by n_res.

Mutants are computed on the float64 restatement alone (windowed_forward); project code is
never made wrong.  No tolerance is introduced here: the stage bars are test_gpu_stages.py's,
the wav bar the project's 1e-4.
"""
import functools
from dataclasses import dataclass

import numpy as np
import torch

from dynamic_range_cases import Block, V1_D, V1_K, V2_D, V2_K, block_convs
from oracle import config as C
from oracle import hifigan_np64 as N
from oracle import prng
from test_gpu_stages import STAGE_RTOL, stage_bar  # noqa: F401  (the only stage tolerances used)
from width_cases import BF16X3_TILES

ATOL = 1e-4   # the project's wav bar
SPLIT_PRECISIONS = ("f16x3", "bf16x3", "bf16w")
PRECISIONS = ("fp32",) + SPLIT_PRECISIONS
# bf16w: scaled-f16 activations on bf16-stored weights; the probe weights are bf16-exact, so it
# computes the reference model with f16x3's arithmetic and gets f16x3's bar
RTOL = dict(STAGE_RTOL, bf16w=STAGE_RTOL["f16x3"])
WIDEST = "bf16x3"   # the widest stage bar any precision gets
V3_K, V3_D = V2_K, V2_D   # the release V3 lists (tests/release_oracle.py, synth.RELEASE_V3)
# NTILE of the fp32 layer kernel's tiles (kernels.h kTiles: 32 WN WAVES_N)
FP32_NTILE = {0: 128, 1: 256, 2: 512}


# ----------------------------------------------------------------------------------------
# the probe handles: one per launch under test
# ----------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    blk: Block
    launch: str    # what the f16x3 plan must run: "fused", "split", "rb2", "thin", "thin_mfma", "layer"
    nwin: int = 0  # the window the plan must report (0: not pinned here)

    @property
    def name(self):
        return self.blk.name


def _rb(name, ch, j, seed, kernels=V1_K, dils=V1_D, rb="1"):
    return Block(name, ch, kernels, dils, rb, j=j, seed=seed)


CASES = [
    # whole-ResBlock launches (resblock_bf16x3); k = 11 at C <= 64 is split in two by default
    Case(_rb("c32_k3", 32, 0, 401), "fused", 512),
    Case(_rb("c32_k7", 32, 1, 402), "fused", 512),
    Case(_rb("c32_k11", 32, 2, 403), "split", 512),
    Case(_rb("c64_k3", 64, 0, 404), "fused", 256),      # the 256-column C = 64 window
    Case(_rb("c64_k7", 64, 1, 405), "fused", 512),
    Case(_rb("c64_k11", 64, 2, 406), "split", 512),
    Case(_rb("c128_k3", 128, 0, 407), "fused", 256),
    # C = 128, k = 7 / 11: the halo recompute is over the planner's 15 %, layer launches
    Case(_rb("c128_k7", 128, 1, 408), "layer"),
    Case(_rb("c128_k11", 128, 2, 409), "layer"),
    # ResBlock2 (resblock2_bf16x3), the V3 lists; C = 128 has a whole-block instance for k = 3
    Case(_rb("rb2_c32_k3", 32, 0, 411, V3_K, V3_D, "2"), "rb2", 512),
    Case(_rb("rb2_c32_k5", 32, 1, 412, V3_K, V3_D, "2"), "rb2", 512),
    Case(_rb("rb2_c32_k7", 32, 2, 413, V3_K, V3_D, "2"), "rb2", 512),
    Case(_rb("rb2_c64_k3", 64, 0, 414, V3_K, V3_D, "2"), "rb2", 256),
    Case(_rb("rb2_c64_k7", 64, 2, 415, V3_K, V3_D, "2"), "rb2", 512),
    Case(_rb("rb2_c128_k3", 128, 0, 416, V3_K, V3_D, "2"), "rb2", 256),
    # thin whole-MRF launches (V2*'s last stages)
    Case(Block("thin_c8", 8, V2_K, V2_D, seed=421), "thin"),
    Case(Block("thin_c16", 16, V2_K, V2_D, seed=422), "thin_mfma"),
    # the layer path on the A-in-registers tiles and on the small tile
    Case(_rb("c256_k3", 256, 0, 431), "layer"),
    Case(_rb("c512_k7", 512, 0, 432, (7,), ((1, 3),)), "layer"),
]
BY_NAME = {c.name: c for c in CASES}
MAX_LAYER_COLS = 600   # C = 256 / 512: the float64 reference stays under a second


def knob_sets(case):
    """The schedule overrides the GPU test runs a case under, the default schedule first: the
    whole-block kernels under FUSED_RB 1 and 0 and RB_SPLIT 1 and 0, the layer path under
    SMALL_TILE 0 and 1."""
    return {"fused": [{}, {"RB_SPLIT": 0}, {"FUSED_RB": 0}],
            "split": [{}, {"RB_SPLIT": 0}, {"FUSED_RB": 0}],
            "rb2": [{}, {"FUSED_RB": 0}],
            "thin": [{}], "thin_mfma": [{}],
            "layer": [{"SMALL_TILE": 0}, {"SMALL_TILE": 1}]}[case.launch]


def radius(k, d):
    return (k - 1) // 2 * d


def case_convs(blk, j):
    """[(state-dict prefix, k, dilation, second conv of a pair)] of ResBlock j in execution
    order."""
    out = []
    for i, (pre, d) in enumerate(block_convs(blk, j)):
        out.append((pre, blk.kernels[j], d, blk.resblock != "2" and i % 2 == 1))
    return out


# ----------------------------------------------------------------------------------------
# probe weights and inputs
# ----------------------------------------------------------------------------------------
def shift_conv(seed, key, channels, k, bias_scale=1.0, c_out=None):
    """(weight [C_out, C, k], bias [C_out]) float32 of one probe conv: a 1 on tap 0 from
    channel pi(co) and on tap k - 1 from channel pi(co) + 1; bias in {0, bias_scale}."""
    c_out = channels if c_out is None else c_out
    pi = np.argsort(prng.uniform01(seed, key + "#pi", channels))[np.arange(c_out) % channels]
    w = np.zeros((c_out, channels, k), np.float32)
    w[np.arange(c_out), pi, 0] = 1.0
    w[np.arange(c_out), (pi + 1) % channels, k - 1] = 1.0
    b = (prng.uniform01(seed, key + "#b", c_out) < 0.5).astype(np.float32) * np.float32(bias_scale)
    return w, b


@functools.lru_cache(maxsize=None)
def probe_state(blk, bias_scale=1.0):
    """Probe weights under the MRF module's own state_dict keys (shared: never modified)."""
    sd = {}
    for j in range(len(blk.kernels)):
        for pre, k, _, _ in case_convs(blk, j):
            sd[pre + ".weight"], sd[pre + ".bias"] = shift_conv(blk.seed, pre, blk.channels, k,
                                                               bias_scale)
    for v in sd.values():
        v.setflags(write=False)
    return sd


@functools.lru_cache(maxsize=None)
def default_state(blk):
    """The same keys with the default-init weights of V1's ResBlocks
    (oracle.config.make_state_dict(V1, seed = 0), the stage of this width; widths V1 has no
    stage for: PRNG weights at the same bound)."""
    from dynamic_range_cases import block_state
    stage = {256: 0, 128: 1, 64: 2, 32: 3}.get(blk.channels)
    if stage is None or blk.resblock == "2" or blk.kernels != V1_K:
        return block_state(blk)
    full = C.make_state_dict(C.V1, seed=0)
    return {k[len(f"mrfs.{stage}."):]: v for k, v in full.items() if k.startswith(f"mrfs.{stage}.")}


@functools.lru_cache(maxsize=None)
def probe_input(seed, channels, L, B=2):
    """x f32 [B, C, L], integers in {0 .. 3}."""
    x = np.floor(prng.uniform01(seed, f"x{B}x{L}", B * channels * L) * 4).astype(np.float32)
    x = np.minimum(x, 3).reshape(B, channels, L)
    x.setflags(write=False)
    return x


def make_module(pkg, blk, precision, dev, sd=None):
    """The HIP module of the case: the MRF, or its ResBlock j."""
    mrf = pkg.MRF(blk.channels, list(blk.kernels), [list(d) for d in blk.dilations],
                  precision=precision, resblock=blk.resblock).eval()
    mrf.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in (sd or probe_state(blk)).items()})
    mrf = mrf.to(dev)
    return mrf if blk.j < 0 else mrf.resblocks[blk.j]


# ----------------------------------------------------------------------------------------
# float64 references
# ----------------------------------------------------------------------------------------
def reference(blk, x, sd=None):
    """float64 [B, C, L] of the case's module on x (oracle/hifigan_np64.py)."""
    f = sd or probe_state(blk)
    if blk.j < 0:
        return N.mrf_forward(f, "", x, blk.kernels, blk.dilations, blk.resblock)
    return N.resblock_forward(f, f"resblocks.{blk.j}", x, blk.kernels[blk.j], blk.dilations[blk.j],
                              blk.resblock)


@functools.lru_cache(maxsize=None)
def probe_ref(name, L, B=2):
    """(x, float64 reference) of a case at length L; computed once per session and shared."""
    blk = BY_NAME[name].blk
    x = probe_input(blk.seed, blk.channels, L, B)
    ref = reference(blk, x)
    ref.setflags(write=False)
    return x, ref


def _conv(f, pre, x, k, d):
    return N.conv1d(x, np.asarray(f[pre + ".weight"], np.float64),
                    np.asarray(f[pre + ".bias"], np.float64), C.get_padding(k, d), d)


def windowed_forward(f, convs, x, length, W, halo, first_exact, *, short=(0, 0), shift=0,
                     unmasked=(), post=None):
    """One block (`convs`: case_convs, or a slice of it for one part of a split launch) computed
    window by window the way the kernels do, in float64.  Window i keeps columns [i W, i W + W)
    and holds [i W - halo, i W + W + halo); with first_exact the first conv reads its radius of
    x beyond the window and is exact on all of it (resblock_bf16x3, RbConvs::halo), otherwise
    every conv sees the window alone (mrf_thin: halo = all radii).  Each later conv reads zeros
    outside the window, and its input is zeroed outside [0, length).

    With the defaults and halo >= the launch's tap reach this is the unwindowed block, exactly.
    The mutants: short = (l, r) columns missing from the halo on either side; shift: the window
    is loaded `shift` columns to the right of where its results are stored; unmasked: indices
    of convs whose input is not zeroed past `length`.
    post = (others, n_res, w, b): the fused conv_post launch: the stage (others + block) / n_res
    on the window, then tanh(conv_post(lrelu(stage, 0.1))) kept on the centre; returns the wav.
    """
    x = np.asarray(x, np.float64)
    Bn, Cn, L = x.shape
    hl, hr = halo - short[0], halo - short[1]
    r0 = radius(convs[0][1], convs[0][2]) if first_exact else 0
    out = np.zeros((Bn, 1 if post else Cn, length))
    rb2 = not any(s for *_, s in convs)
    for t0 in range(0, length, W):
        a, b = t0 - hl + shift, t0 + W + hr + shift
        cols = np.arange(a - r0, b + r0)
        ve = (cols >= 0) & (cols < length)
        xe = np.where(ve, x[..., np.clip(cols, 0, L - 1)], 0.0)
        valid = ve[r0:r0 + b - a].astype(np.float64)
        front = (cols[r0:r0 + b - a] >= 0).astype(np.float64)   # an unmasked end keeps its start
        xr = xe[..., r0:r0 + b - a]
        xt = None
        for i, (pre, k, d, second) in enumerate(convs):
            if i == 0 and first_exact:
                y = _conv(f, pre, N.lrelu(xe), k, d)[..., r0:r0 + b - a]
            else:
                m = front if i in unmasked else valid
                y = _conv(f, pre, N.lrelu(xt if second else xr) * m, k, d)
            if second or rb2:
                xr = xr + y
            else:
                xt = y
        n = min(W, length - t0)
        if post:
            others, n_res, pw, pb = post
            oc = np.where(ve[r0:r0 + b - a], others[..., np.clip(cols[r0:r0 + b - a], 0, length - 1)], 0.0)
            stage = (oc + xr) / n_res
            wav = np.tanh(N.conv1d(N.lrelu(stage) * valid, pw, pb, 3, 1))
            out[..., t0:t0 + n] = wav[..., hl:hl + n]
        else:
            out[..., t0:t0 + n] = xr[..., hl:hl + n]
    return out


def swapped(convs, rb2):
    """Mutant (d): the dilations of every pair swapped (conv1 runs at 1, conv2 at d); a
    ResBlock2's dilation list reversed."""
    if rb2:
        ds = [d for _, _, d, _ in convs][::-1]
        return [(p, k, d, s) for (p, k, _, s), d in zip(convs, ds)]
    out = []
    for i in range(0, len(convs), 2):
        (p1, k, d1, _), (p2, _, d2, _) = convs[i], convs[i + 1]
        out += [(p1, k, d2, False), (p2, k, d1, True)]
    return out


# ----------------------------------------------------------------------------------------
# window geometry from the plan dump
# ----------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Window:
    tag: str          # "whole", "part0", "part1", "post", "thin", "thin_mfma", "tile", "small", "fp32"
    j: int            # the ResBlock of the handle it belongs to (thin / layer: 0)
    conv0: int        # its convs [conv0, conv1) of case_convs
    conv1: int
    W: int
    halo: int
    nwin: int
    r_max: int
    first_exact: bool

    @property
    def windowed(self):
        return self.halo > 0


def window_width(nwin, halo):
    """plan.cpp window_width (pinned against the dump by test_seams_host.py)."""
    W = (nwin - 2 * halo) & ~3
    return W if W >= nwin // 4 else 0


def _host_handle(pkg, blk, precision, sd):
    ks = list(blk.kernels) if blk.j < 0 else [blk.kernels[blk.j]]
    ds = [list(d) for d in blk.dilations] if blk.j < 0 else [list(blk.dilations[blk.j])]
    h = pkg.Handle(pkg._lib.make_mrf_config(blk.channels, ks, ds, precision=precision,
                                            resblock=blk.resblock), -1, mrf=True)
    for jj, j in enumerate(blk.blocks):
        for pre, _ in block_convs(blk, j):
            tail = pre.split(".", 2)[2]
            for leaf in (".weight", ".bias"):
                h.set_weight(f"resblocks.{jj}.{tail}{leaf}", torch.from_numpy(np.array(sd[pre + leaf])))
    h.commit()
    return h


def host_plan(pkg, blk, precision="f16x3"):
    """hfg_debug_plan of a host-only handle of the case with its probe weights committed, under
    whatever schedule overrides are in force."""
    return _host_handle(pkg, blk, precision, probe_state(blk)).plan()


def _layer_windows(plan32, plan16, j, n, r_max):
    """The layer-per-launch tiles of a block: every conv is its own launch with no halo; a tile
    of NTILE columns is its "window".  The first split-precision conv of the f16x3 plan names
    the split tiles (a block may mix in convs past the split kernel's reach, which run the fp32
    kernel inside a split handle)."""
    out = []
    L16 = next((L for L in plan16["layers"] if L["prec"] == 1), None)
    L32 = plan32["layers"][0]
    if L16:
        out.append(("tile", 32 * BF16X3_TILES[L16["tile"]][4] * BF16X3_TILES[L16["tile"]][2]))
        if L16["small"][0] >= 0:
            t = BF16X3_TILES[L16["small"][0]]
            out.append(("small", 32 * t[4] * t[2]))
    out.append(("fp32", FP32_NTILE[L32["tile"]]))
    return [Window(tag, j, 0, n, nt, 0, nt, r_max, True) for tag, nt in out]


def windows(pkg, name):
    """block_windows of a case of this file."""
    return block_windows(pkg, BY_NAME[name].blk)


@functools.lru_cache(maxsize=None)
def block_windows(pkg, blk):
    """Every launch geometry the block's handle can run, from hfg_debug_plan of its f16x3 and
    fp32 plans under the default schedule: the whole-block window, both parts of a split one,
    the thin kernels' (hfg_debug_thin_window), and the NTILE of the layer launches that
    FUSED_RB 0, SMALL_TILE 1 and the fp32 precision run instead."""
    assert not pkg.schedule_overrides(), "window geometry is the default schedule's"
    p16, p32 = host_plan(pkg, blk, "f16x3"), host_plan(pkg, blk, "fp32")
    st = p16["stages"][0]
    out = []
    if st["thin"] or p32["stages"][0]["thin"]:
        lib = pkg.load_library()
        halo = max(st["thin_halo"])
        r_max = max(radius(k, d) for j in blk.blocks for _, k, d, _ in case_convs(blk, j))
        for tag, mf, on in (("thin", 0, True), ("thin_mfma", 1, st["thin_mfma"])):
            nwin = lib.hfg_debug_thin_window(blk.channels, mf)
            if on and nwin > 0:
                out.append(Window(tag, -1, 0, 0, nwin - 2 * halo, halo, nwin, r_max, False))
        return tuple(out)
    for jj, j in enumerate(blk.blocks):
        convs = case_convs(blk, j)
        rad = [radius(k, d) for _, k, d, _ in convs]
        rb = st["rbs"][jj]
        if rb["fused"]:
            out.append(Window("whole", j, 0, len(convs), rb["W"], rb["halo"], rb["nwin"], max(rad), True))
            if rb["split"]:
                h0, h1, w0, w1 = rb["parts"]
                s = rb["split"]
                out.append(Window("part0", j, 0, s, w0, h0, rb["nwin"], max(rad[:s]), True))
                out.append(Window("part1", j, s, len(convs), w1, h1, rb["nwin"], max(rad[s:]), True))
        out += _layer_windows(p32, p16, j, len(convs), max(rad))
    return tuple(out)


CLASSES = ("1", "r_max", "halo", "halo+1", "W-1", "W", "W+1", "W+halo-1", "W+halo", "W+halo+1",
           "nwin-1", "nwin", "nwin+1", "2W-1", "2W", "2W+1", "2W+halo+2")


def length_classes(w):
    """{class: L} of one launch geometry (the issue's list)."""
    W, h, n = w.W, w.halo, w.nwin
    return dict(zip(CLASSES, (1, w.r_max, h, h + 1, W - 1, W, W + 1, W + h - 1, W + h, W + h + 1,
                              n - 1, n, n + 1, 2 * W - 1, 2 * W, 2 * W + 1, 2 * W + h + 2)))


def block_max_length(pkg, blk):
    """L <= 2 nwin + 64 of the block's largest window; C = 256 / 512: <= 600 columns."""
    if blk.channels >= 256:
        return MAX_LAYER_COLS
    return 2 * max(w.nwin for w in block_windows(pkg, blk)) + 64


def block_lengths(pkg, blk):
    """Sorted lengths of a block: every class of every launch geometry of its handle that is a
    length (>= 1) within block_max_length."""
    cap = block_max_length(pkg, blk)
    return sorted({L for w in block_windows(pkg, blk) for L in length_classes(w).values()
                   if 1 <= L <= cap})


def max_length(pkg, name):
    return block_max_length(pkg, BY_NAME[name].blk)


def lengths(pkg, name):
    return block_lengths(pkg, BY_NAME[name].blk)


def seams(w, length):
    """Columns where a window of this geometry starts (t0 > 0) within [0, length)."""
    return list(range(w.W, length, w.W))


def seam_distance(ws, t, length):
    """(distance, what) of column t to the nearest seam of any of the windows `ws`, or to the
    end of the sequence."""
    best = (length - 1 - t, "end")
    for w in ws:
        for s in seams(w, length):
            d = t - s if t >= s else s - 1 - t
            if d < best[0]:
                best = (d, f"{w.tag} seam at {s}")
    return best


# ----------------------------------------------------------------------------------------
# mutants of one launch geometry
# ----------------------------------------------------------------------------------------
def mutant_length(w, cap):
    """Three windows and a ragged end where that fits, else two."""
    L = 2 * w.W + w.halo + 2
    return L if L <= cap else w.W + w.halo + 1


def block_mutants(blk, w, x, f=None):
    """{mutant: (float64 output, columns allowed to move [bool, L])} of window geometry `w` of a
    ResBlock case on x, `length` = x's.  A split part is fed / followed by the exact other part.
    The allowed columns: (a) within halo of a seam, on the side the halo is short; (b), (d)
    anywhere; (c) within the reach of the convs from the unmasked one on of the end."""
    f = f or probe_state(blk)
    L = x.shape[-1]
    convs = case_convs(blk, w.j)
    rb2 = blk.resblock == "2"
    mine = convs[w.conv0:w.conv1]
    t = np.arange(L)

    def run(**kw):
        xin = x
        if w.conv0:   # the exact first part
            xin = windowed_forward(f, convs[:w.conv0], x, L, L, 0, True)
        y = windowed_forward(f, mine, xin, L, w.W, w.halo, w.first_exact, **kw)
        if w.conv1 < len(convs):
            y = windowed_forward(f, convs[w.conv1:], y, L, L, 0, True)
        return y

    rest = sum(radius(k, d) for _, k, d, _ in convs[w.conv1:])   # reach of the part after
    near = np.zeros(L, bool)
    left, right = near.copy(), near.copy()
    for s in seams(w, L):
        left |= (t >= s - rest) & (t < s + w.halo + rest)
        right |= (t >= s - w.halo - rest) & (t < s + rest)
    reach = [sum(radius(k, d) for _, k, d, _ in convs[i:]) for i in range(len(convs))]
    n = len(mine)
    everywhere = np.ones(L, bool)
    out = {"exact": (run(), near),
           "a:left": (run(short=(1, 0)), left), "a:right": (run(short=(0, 1)), right),
           "b:origin": (run(shift=1), everywhere),
           "c:all": (run(unmasked=tuple(range(1, n))), t >= L - reach[w.conv0 + 1]),
           "c:last": (run(unmasked=(n - 1,)), t >= L - reach[w.conv0 + n - 1])}
    sw = swapped(convs, rb2)
    out["d:swap"] = (windowed_forward(f, sw, x, L, L, 0, True), everywhere)
    return out


def thin_mutants(blk, w, x, f=None):
    """The same for a thin whole-MRF launch: every block on the launch's one window (halo = the
    largest block's summed radii, no exact first conv), then the mean."""
    f = f or probe_state(blk)
    L = x.shape[-1]
    t = np.arange(L)
    n_res = len(blk.kernels)
    chains = [case_convs(blk, j) for j in range(n_res)]

    def run(swap=False, **kw):
        acc = 0.0
        for convs in chains:
            um = kw.get("unmasked")
            k2 = dict(kw)
            if um == "all":
                k2["unmasked"] = tuple(range(len(convs)))
            elif um == "last":
                k2["unmasked"] = (len(convs) - 1,)
            acc = acc + windowed_forward(f, swapped(convs, False) if swap else convs, x, L, w.W,
                                         w.halo, False, **k2)
        return acc / n_res

    left, right = np.zeros(L, bool), np.zeros(L, bool)
    for s in seams(w, L):
        left |= (t >= s) & (t < s + w.halo)
        right |= (t >= s - w.halo) & (t < s)
    reach_all = max(sum(radius(k, d) for _, k, d, _ in c) for c in chains)
    reach_last = max(radius(c[-1][1], c[-1][2]) for c in chains)
    everywhere = np.ones(L, bool)
    return {"exact": (run(), np.zeros(L, bool)),
            "a:left": (run(short=(1, 0)), left), "a:right": (run(short=(0, 1)), right),
            "b:origin": (run(shift=1), everywhere),
            "c:all": (run(unmasked="all"), t >= L - reach_all),
            "c:last": (run(unmasked="last"), t >= L - reach_last),
            "d:swap": (run(swap=True), everywhere)}


def mutants(blk, w, x, f=None):
    return (thin_mutants if w.j < 0 else block_mutants)(blk, w, x, f)


MUTANTS = ("a:left", "a:right", "b:origin", "c:all", "c:last", "d:swap")


# ----------------------------------------------------------------------------------------
# generators with a probe tail
# ----------------------------------------------------------------------------------------
GEN_CONFIGS = {"v1": C.V1, "v2star": C.V2STAR}
GEN_SEED = 441
GEN_T = 4                       # frames: L = 256 T = 1024 <= 2 nwin + 64
GEN_LENS = (4, 3, 2, 1)         # last-stage lengths 1024, 768, 512, 256
GEN_BIAS = 2.0 ** -5            # probe biases at the scale of the default-init stage input
POST_TAPS = ((0, 0, 1.0), (1, 6, -1.0), (2, 3, 0.5), (3, 0, -0.5))   # (channel, tap, sign x 2^-n)


def gen_blk(name):
    cfg = GEN_CONFIGS[name]
    ch = cfg.upsample_initial_channel >> len(cfg.upsample_rates)
    return Block(f"{name}_tail", ch, tuple(cfg.resblock_kernel_sizes),
                 tuple(tuple(d) for d in cfg.resblock_dilation_sizes), seed=GEN_SEED)


@functools.lru_cache(maxsize=None)
def gen_mel(name):
    m = prng.mel_input(GEN_SEED, (len(GEN_LENS), GEN_CONFIGS[name].n_mels, GEN_T))
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def gen_state(name):
    """Default-init weights up to the last upsampler, probe weights (biases in {0, 2^-5}) in the
    last MRF, and in conv_post a signed power-of-two pattern on four (channel, tap) pairs at the
    scale 2^-p that keeps |pre-tanh| <= 1 on the test's mel (p from the float64 reference)."""
    cfg = GEN_CONFIGS[name]
    last = len(cfg.upsample_rates) - 1
    sd = {k: np.array(v) for k, v in C.make_state_dict(cfg, seed=GEN_SEED).items()}
    for k, v in probe_state(gen_blk(name), GEN_BIAS).items():
        assert sd[f"mrfs.{last}.{k}"].shape == v.shape
        sd[f"mrfs.{last}.{k}"] = np.array(v)
    sd["conv_post.weight"][:] = 0.0
    sd["conv_post.bias"][:] = 0.0
    box = {}
    N.generator_forward(sd, cfg, gen_mel(name), tap=lambda n, t: box.__setitem__(n, t))
    top = float(np.abs(N.lrelu(box[f"mrfs.{last}"])).max()) * sum(abs(s) for *_, s in POST_TAPS)
    p = int(np.ceil(np.log2(top)))
    for ch, tap, s in POST_TAPS:
        sd["conv_post.weight"][0, ch, tap] = np.float32(s * 2.0 ** -p)
    for v in sd.values():
        v.setflags(write=False)
    return sd


def make_generator(pkg, name, precision, dev):
    gen = pkg.HiFiGANGenerator(**GEN_CONFIGS[name].kwargs(), precision=precision).eval()
    gen.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in gen_state(name).items()})
    return gen.to(dev)


@functools.lru_cache(maxsize=None)
def gen_host_plan(pkg, name, precision="f16x3"):
    h = pkg.Handle(pkg.make_config(**GEN_CONFIGS[name].kwargs(), precision=precision), -1)
    for k, v in gen_state(name).items():
        h.set_weight(k, torch.from_numpy(np.array(v)))
    h.commit()
    return h.plan()


@functools.lru_cache(maxsize=None)
def gen_refs(name, b=None, n=None):
    """({tap: float64}, {tap: fp32 oracle as float64}) of the whole mel, "wav" included; with
    b / n: of item b alone on its first n frames."""
    from oracle import hifigan_torch as H
    cfg, sd = GEN_CONFIGS[name], gen_state(name)
    m = np.array(gen_mel(name))
    if b is not None:
        m = m[b:b + 1, :, :n]
    r64, r32 = {}, {}
    r64["wav"] = N.generator_forward(sd, cfg, m, tap=lambda k, t: r64.__setitem__(k, t.copy()))
    r32["wav"] = H.generator_forward(
        H.to_torch_state({k: np.array(v) for k, v in sd.items()}), cfg, torch.from_numpy(m),
        tap=lambda k, t: r32.__setitem__(k, t.numpy().astype(np.float64))).numpy().astype(np.float64)
    return r64, r32


def gen_tail_windows(pkg, name):
    """[Window] of the last stage's launches in the Generator's f16x3 plan; the fused conv_post
    launch ("post": halo + 3, W_post = window_width(nwin, halo + 3)) included."""
    blk = gen_blk(name)
    st = gen_host_plan(pkg, name)["stages"][-1]
    out = []
    if st["thin"]:
        nwin = pkg.load_library().hfg_debug_thin_window(blk.channels, 1 if st["thin_mfma"] else 0)
        halo = max(st["thin_halo"])
        r_max = max(radius(k, d) for j in blk.blocks for _, k, d, _ in case_convs(blk, j))
        return [Window("thin_mfma" if st["thin_mfma"] else "thin", -1, 0, 0, nwin - 2 * halo, halo,
                       nwin, r_max, False)]
    for j, rb in enumerate(st["rbs"]):
        convs = case_convs(blk, j)
        rad = [radius(k, d) for _, k, d, _ in convs]
        assert rb["fused"], (name, j)
        s, n = rb["split"], len(convs)
        if s:
            h0, h1, w0, w1 = rb["parts"]
            out.append(Window("part0", j, 0, s, w0, h0, rb["nwin"], max(rad[:s]), True))
            out.append(Window("part1", j, s, n, w1, h1, rb["nwin"], max(rad[s:]), True))
        else:
            out.append(Window("whole", j, 0, n, rb["W"], rb["halo"], rb["nwin"], max(rad), True))
        if rb["post"]:
            hp = (rb["parts"][1] if s else rb["halo"]) + 3
            out.append(Window("post", j, s, n, window_width(rb["nwin"], hp), hp, rb["nwin"],
                              max(rad[s:]), True))
    return out
