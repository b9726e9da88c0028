"""Channel widths off the power-of-two grid, on the CPU (tests/width_cases.py): every
configuration is accepted in every precision and reaches the kernel paths it exists for (a
planner change that moves one fails here), every layer's packed image — the layer's own tile,
the small-tile packing, the output-frame upsampler's — holds exactly the state dict's weights
(or their hi / lo split at the reported exponent) with every padded row, channel, tap and bias
entry zero, the packed GEMM reproduces the convolution, and the stage bars of the GPU tests
resolve a wrong tail channel or tail row of the float64 reference by a wide margin."""
import functools

import numpy as np
import pytest
import torch

import width_cases as W
from oracle import config as C
from oracle import hifigan_np64 as N
from test_capi_host import (SPLIT_TOL, WAVES, _bf16_rne, _scatter, config_layers, dec,
                            emulate_conv, unpack_bf16x3_planes, unpack_gemm_padded)

NAMES = list(W.CONFIGS)
UPS_WAVES = {0: (2, 1), 1: (1, 1)}   # kUpsCfgs: configuration -> (WAVES_M, WM)


@functools.lru_cache(maxsize=None)
def handle(pkg, name, precision):
    return W.host_handle(pkg, name, precision)


@functools.lru_cache(maxsize=None)
def plan(pkg, name, precision):
    return handle(pkg, name, precision).plan()


# ----------------------------------------------------------------------------------------
# acceptance and coverage
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", W.PRECISIONS)
@pytest.mark.parametrize("name", NAMES)
def test_config_is_accepted(pkg, name, precision):
    cfg = W.CONFIGS[name]
    h = handle(pkg, name, precision)
    for t in (1, 3, 33, 40):
        assert h.out_len(t) == C.out_len(cfg, t)
    for b, t in ((1, 1), (3, 40)):
        assert h.workspace_bytes(b, t) > 0
    p = plan(pkg, name, precision)
    assert [st["C"] for st in p["stages"]] == \
        [cfg.upsample_initial_channel >> (i + 1) for i in range(len(cfg.upsample_rates))]
    for st in p["stages"]:   # no whole-block kernel (C in {32, 64, 128}) and no thin one (8, 16)
        assert st["thin"] == 0 and all(rb["fused"] == 0 for rb in st["rbs"]), st
    assert [L["mod"] for L in p["layers"]] == [m for m, *_ in config_layers(cfg)] + ["conv_post"]


def test_w200r_runs_conv_post_at_an_odd_length():
    cfg = W.CONFIGS["W200R"]
    assert C.out_len(cfg, 33) == 15 * 33 and C.out_len(cfg, 33) % 4 != 0
    assert cfg.upsample_initial_channel >> 2 == 50


@pytest.mark.parametrize("target", W.TARGETS,
                         ids=[f"{t.config}-{t.precision}-{t.layers}" for t in W.TARGETS])
def test_coverage_target_is_reached(pkg, target):
    layers = target.matches(plan(pkg, target.config, target.precision))
    assert layers, f"{target.layers}: no such layer"
    for L in layers:
        got = {k: W.layer_field(L, k) for k, _ in target.want}
        assert target.holds(L), f"{L['mod']} left its path ({target.why}): {got} != {dict(target.want)}"


def test_every_config_has_targets_in_both_kernel_families():
    for name in NAMES:
        assert W.targets(name, "f16x3") and W.targets(name, "fp32"), name


# ----------------------------------------------------------------------------------------
# packing of every layer
# ----------------------------------------------------------------------------------------
def gemm_weight(w, kind, u, KT):
    """The GEMM operand wt[row][ci][tap] (float32) of a layer, unpadded.  Conv1d: its weight
    [C_out][C_in][k].  Polyphase ConvTranspose1d (weight [C_in][C_out][k]): row = co u + r, tap
    jj holds kernel index r + u (KT - 1 - jj), zero where that is past k."""
    if kind == 0:
        return np.array(w, np.float32)
    cin, cout, k = w.shape
    E = np.zeros((cout * u, cin, KT), np.float32)
    for r in range(u):
        for jj in range(KT):
            kidx = r + u * (KT - 1 - jj)
            if kidx < k:
                E[r::u, :, jj] = w[:, :, kidx].T
    return E


def padded(E, shape):
    out = np.zeros(shape, E.dtype)
    out[:E.shape[0], :E.shape[1], :E.shape[2]] = E
    return out


def split_planes(E, precision, ew):
    """(hi, lo) of pack.cpp's split_w as float64, from float32 E: bf16x3 hi = bf16(w), lo =
    bf16(w - hi); f16x3 / bf16w hi = f16(w 2^ew), lo = f16(w 2^ew - hi), both times 2^-ew."""
    if precision == "bf16x3":
        hi = _bf16_rne(E)
        return hi.astype(np.float64), _bf16_rne(E - hi).astype(np.float64)
    a = E * np.float32(2.0 ** ew)
    hi = a.astype(np.float16)
    lo = (a - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64) * 2.0 ** -ew, lo.astype(np.float64) * 2.0 ** -ew


def check_packing(h, mod, W_, bias, kind, u, precision):
    """One packing (`mod`, or `mod#small`) against the state dict; returns (info, unpacked
    operand float64 [M][C_in][KT], per-row bias)."""
    info, packed, brow = h.packed_layer(mod)
    M, KT = info["M"], info["KT"]
    E = gemm_weight(W_, kind, u, KT)
    assert E.shape[0] == M and info["kind"] == kind
    cin = E.shape[1]
    if info["CK"] == 16 and precision != "fp32":
        hi, lo = unpack_bf16x3_planes(info, packed, WAVES[info["tile"]], precision)
        want_hi, want_lo = split_planes(padded(E, hi.shape), precision, info["ew"])
        assert hi.shape[0] >= M and hi.shape[1] >= cin and hi.shape[2] >= KT
        # equality of the whole padded operand: padded rows, channels and taps are zero
        assert np.array_equal(hi, want_hi), f"{mod}: hi plane"
        assert np.array_equal(lo, want_lo), f"{mod}: lo plane"
        assert not hi[M:].any() and not hi[:, cin:].any() and not hi[:, :, KT:].any(), mod
        assert not lo[M:].any() and not lo[:, cin:].any() and not lo[:, :, KT:].any(), mod
        if precision != "bf16x3":  # the layer's max |w| lands in [2^14, 2^15) of f16
            assert info["ew"] == 15 - int(np.frexp(np.abs(W_).max())[1]), mod
        if precision == "bf16w":
            assert not lo.any(), f"{mod}: lo plane of bf16-valued weights"
        Wt = hi + lo
    else:
        Wt = unpack_gemm_padded(info, packed)
        assert np.array_equal(Wt, padded(E, Wt.shape).astype(np.float64)), mod
        assert not Wt[M:].any() and not Wt[:, cin:].any(), mod
        assert info["ew"] == 0 or precision in ("f16x3", "bf16w")
    # per-row bias: bias[row // u] on the M rows, zero on the padding of the last m-tile
    assert len(brow) == info["m_tiles"] * info["MT"] >= M
    assert np.array_equal(brow[:M], np.repeat(bias, u)), mod
    assert not brow[M:].any(), f"{mod}: bias padding"
    return info, Wt[:M, :cin, :KT], brow


def check_frames_packing(h, mod, W_, bias, u, precision, frames):
    """The output-frame upsampler's packing (pack.cpp pack_ups_frames): class L rows (samples
    s' < u/2 of a frame) taps x[m-1], x[m] = kernel indices s'+h+u, s'+h; class R taps x[m],
    x[m+1] = s'+u, s'."""
    info, packed, b = h.packed_layer(mod + "#frames")
    cin, cout, k = W_.shape
    hh = u // 2
    wm_, WM = UPS_WAVES[info["tile"]]
    MT = info["MT"]
    assert (info["tile"], info["m_tiles"]) == frames and MT == 32 * WM * wm_ and k == 2 * u
    assert info["M"] == cout * hh == info["m_tiles"] * MT and info["n_chunks"] * 16 == cin
    shape = (info["m_tiles"], cin // 16, 2, 2, wm_, WM, 64, 8)
    raw = packed.view(np.uint16).reshape(shape[:4] + (2,) + shape[4:])
    mt, g, c, tp, wv, wm, lane, e = np.ogrid[tuple(slice(0, n) for n in shape)]
    idx = (mt * MT + wv * 32 * WM + wm * 32 + (lane & 31), g * 16 + 8 * (lane >> 5) + e, c * 2 + tp)
    E = np.zeros((cout * hh, cin, 4), np.float32)
    for rr in range(cout * hh):
        co, sp = divmod(rr, hh)
        for slot, j in enumerate((sp + hh + u, sp + hh, sp + u, sp)):
            E[rr, :, slot] = W_[:, co, j]
    want = split_planes(E, precision, info["ew"])
    for plane in (0, 1):
        got = _scatter(E.shape, dec(raw[:, :, :, :, plane], precision, info["ew"]), *idx)
        assert np.array_equal(got, want[plane]), f"{mod}#frames plane {plane}"
    assert np.array_equal(b, bias), f"{mod}#frames bias"


def emulation_bound(precision, W_, cin_k, x):
    """|emulated - float64 conv| allowed: the unpacked operand differs from the weights by at
    most SPLIT_TOL relative to max|w| per element (bf16 halves ~2^-16, scaled f16 halves
    ~2^-22; fp32 and bf16w images are exact: 2^-40 covers the float64 summation), summed over
    C_in k products of magnitude <= max|x|."""
    tol = SPLIT_TOL["bf16x3"] if precision == "bf16x3" else \
        SPLIT_TOL["f16x3"] if precision == "f16x3" else 2.0 ** -40
    return tol * float(np.abs(W_).max()) * cin_k * float(np.abs(x).max())


@pytest.mark.parametrize("precision", W.PRECISIONS)
@pytest.mark.parametrize("name", NAMES)
def test_packing_of_every_layer(pkg, name, precision):
    cfg, sd = W.CONFIGS[name], W.state(name)
    if precision == "bf16w":
        sd = W.bf16_rounded(sd)
    h = handle(pkg, name, precision)
    by_mod = {L["mod"]: L for L in plan(pkg, name, precision)["layers"]}
    rng = np.random.default_rng(7)
    emulated, n_small, n_frames, n_split = set(), 0, 0, 0
    for mod, kind, cin, cout, k, dil, u in config_layers(cfg):
        W_, bias = sd[mod + ".weight"], W.state(name)[mod + ".bias"]
        L = by_mod[mod]
        info, Wt, brow = check_packing(h, mod, W_, bias, kind, u, precision)
        assert (info["tile"], info["m_tiles"], info["n_chunks"]) == \
            (L["tile"], L["m_tiles"], L["n_chunks"])
        n_split += L["prec"]
        if L["small"][0] >= 0:
            small, _, _ = check_packing(h, mod + "#small", W_, bias, kind, u, precision)
            assert (small["tile"], small["m_tiles"], small["n_chunks"]) == tuple(L["small"][:3])
            n_small += 1
        else:
            with pytest.raises(pkg.HfgError):
                h.packed_layer(mod + "#small")
        if L["frames"][0] >= 0:
            check_frames_packing(h, mod, W_, bias, u, precision, tuple(L["frames"][:2]))
            n_frames += 1
        else:
            with pytest.raises(pkg.HfgError):
                h.packed_layer(mod + "#frames")
        # the packed GEMM is the convolution, once per distinct (kind, C_in, M, k, dilation)
        key = (kind, cin, info["M"], k, dil)
        if key in emulated:
            continue
        emulated.add(key)
        w64, b64 = W_.astype(np.float64), bias.astype(np.float64)
        if kind == 0:
            x = rng.standard_normal((cin, 40))
            pad = C.get_padding(k, dil)
            ref = N.conv1d(x[None], w64, b64, pad, dil)[0]
            got = emulate_conv(Wt, brow, x, -pad, dil, 40)
        else:
            x = rng.standard_normal((cin, 13))
            p = (k - u) // 2
            ref = N.conv_transpose1d(x[None], w64, b64, u, p)[0]
            Lout = ref.shape[-1]
            n_cols = (Lout - 1 + p) // u + 1
            g = emulate_conv(Wt, brow, x, -(info["KT"] - 1), 1, n_cols)
            got = np.full((cout, Lout), np.nan)
            for m in range(cout * u):
                co, r = divmod(m, u)
                t = np.arange(n_cols) * u + r - p
                ok = (t >= 0) & (t < Lout)
                got[co, t[ok]] = g[m, ok]
            assert not np.isnan(got).any()
        err = float(np.abs(got - ref).max())
        assert err <= emulation_bound(precision, W_, cin * k, x), (mod, err)
    post, pw, pb = h.packed_layer("conv_post")
    assert post["kind"] == 2
    assert np.array_equal(pw, sd["conv_post.weight"].ravel()) and np.array_equal(pb, sd["conv_post.bias"])
    if precision == "fp32":
        assert n_split == n_small == n_frames == 0
    else:
        want_frames = sum(1 for t in W.targets(name, "f16x3")
                          if dict(t.want).get("frames", (-1, 0))[0] >= 0)
        assert n_split and n_small and n_frames >= want_frames, (n_split, n_small, n_frames)


# ----------------------------------------------------------------------------------------
# the bars can see a tail
# ----------------------------------------------------------------------------------------
class _Reached(Exception):
    pass


def _stage64(name, sd, stage):
    """The float64 oracle's `stage` tensor of the shared mel under weights `sd` (the forward
    stops there)."""
    box = {}

    def tap(n, t):
        if n == stage:
            box["t"] = t.copy()
            raise _Reached

    try:
        N.generator_forward(sd, W.CONFIGS[name], W.mel(name), tap=tap)
    except _Reached:
        pass
    return box["t"]


@pytest.mark.parametrize("name", NAMES)
def test_stage_bars_resolve_a_wrong_tail(name, evidence):
    """A kernel that dropped the last input channel of a partial group, or the last row of a
    partial 32-row block, computes the reference with that channel / row of the weights zero.
    On the float64 oracle alone: zeroing input channel C_in - 1 (and, separately, output row
    M - 1) of one conv per stage moves that stage's output by at least 10 x the widest stage
    bar any precision gets (bf16x3's), so the GPU stage parity cannot pass over such a tail."""
    r64, _ = W.refs(name)
    bars = W.stage_bars(name, "bf16x3")
    worst = None
    for (stage, which), sd in W.tail_mutants(name).items():
        moved = float(np.abs(_stage64(name, sd, stage) - r64[stage]).max())
        ratio = moved / bars[stage][0]
        if worst is None or ratio < worst[0]:
            worst = (ratio, stage, which, moved, bars[stage][0])
        assert ratio >= 10.0, (stage, which, moved, bars[stage])
    evidence(f"{name}: smallest tail move / bf16x3 bar = {worst[0]:.3g} ({worst[1]}, {worst[2]}: "
             f"moved {worst[3]:.3e}, bar {worst[4]:.3e})")
