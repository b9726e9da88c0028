"""Host half of the dynamic-range tests (no GPU; handles are host-only, device = -1).

* The f16x3 layer exponent the host computes for weights (pack.cpp x3_exp_host, read back
  through hfg_debug_layer_exponent) is clamp(15 - frexp_exponent(max|w|), +-60), 0 for an
  all-zero layer, at maxima on, just under and far from a power of two, and the packed hi / lo
  planes reconstruct an outlier layer and a tiny layer to the documented bound.
* Pre-checks of every input test_gpu_dynamic_range.py uses: the float64 reference of each
  quiet region is finite and not identically zero, and the quiet region covers >= 60 % of the
  columns of every spike case.  Those three carry the information.  That the fp32 torch oracle
  meets a regional (or the componentwise) bar is asserted too, but holds by construction: the
  bar contains 4 * cond and cond is that oracle's own error, so the assertion can only fail
  on a non-finite reference.  The one pre-check in which the oracle is held to a bar that does
  not contain its own error is test_subnormal_grid_input.
* The window widths of the thin whole-MRF kernels, which the plan does not list, come from the
  library (hfg_debug_thin_window).
"""
import math

import numpy as np
import pytest
import torch

import dynamic_range_cases as D
from oracle import config as C
from test_capi_host import WAVES, host_handle, unpack_bf16x3

X3_EXP_MAX = 60   # csrc/kernels.h kX3ExpMax
CONV, UPS = "mrfs.0.resblocks.1.convs1.0", "ups.1"


def expected_exponent(w):
    m = float(np.abs(w).max())
    if m == 0.0:
        return 0
    return int(min(max(15 - math.frexp(m)[1], -X3_EXP_MAX), X3_EXP_MAX))


def _weight_variants(w):
    """{name: weights of w's shape} with the maxima of the issue's list."""
    base = w / np.abs(w).max() * np.float32(0.9)   # |base| <= 0.9, one element at 0.9

    def with_max(top):
        v = (base * np.float32(top)).astype(np.float32)
        v.flat[int(np.abs(base).argmax())] = np.float32(top)
        assert float(np.abs(v).max()) == float(np.float32(top))
        return v

    out = {"zero": np.zeros_like(w), "tiny": with_max(2.0 ** -100), "huge": with_max(2.0 ** 100)}
    for k in (-7, 0, 5):
        out[f"pow2_{k}"] = with_max(2.0 ** k)
        out[f"under_pow2_{k}"] = with_max(np.nextafter(np.float32(2.0 ** k), np.float32(0)))
    outlier = w.copy()
    outlier.flat[outlier.size // 3] *= np.float32(2.0 ** 20)
    out["outlier"] = outlier
    return out


def _handle_with(pkg, sd, **replace):
    h = host_handle(pkg, C.V2STAR, "f16x3")
    for k, v in sd.items():
        h.set_weight(k, torch.from_numpy(np.ascontiguousarray(replace.get(k, v))))
    h.commit()
    return h


def _reconstruct(h, mod, shape):
    """The layer's weights from its packed hi + lo planes, times 2^-ew: [cout, cin, k] for a
    conv; for the polyphase ConvTranspose1d (stride u) row co * u + r, tap j of the packed
    GEMM is w[ci, co, (KT - 1 - j) * u + r]."""
    info, packed, _ = h.packed_layer(mod)
    assert info["CK"] == 16, "split layer"
    Wt = unpack_bf16x3(info, packed, WAVES[info["tile"]], "f16x3")
    if info["kind"] == 0:
        cout, cin, k = shape
        return info, Wt[:cout, :cin, :k]
    cin, cout, k = shape
    u, KT = info["M"] // cout, info["KT"]
    rec = np.zeros(shape)
    for j in range(KT):
        for r in range(u):
            kk = (KT - 1 - j) * u + r
            if kk < k:
                rec[:, :, kk] = Wt[r::u, :cin, j][:cout].T
    return info, rec


@pytest.mark.parametrize("mod", [CONV, UPS])
def test_layer_exponent_at_every_maximum(pkg, mod):
    """hfg_debug_layer_exponent == clamp(15 - frexp_exponent(max|w|), +-60); 0 for zeros."""
    sd = C.make_state_dict(C.V2STAR, seed=171)
    seen = set()
    for name, w in _weight_variants(sd[mod + ".weight"]).items():
        h = _handle_with(pkg, sd, **{mod + ".weight": w})
        ew = h.packed_layer(mod)[0]["ew"]
        print(f"{mod} {name}: max|w| {np.abs(w).max():.9g} ew {ew}")
        assert ew == expected_exponent(w), (mod, name, ew, expected_exponent(w))
        seen.add(ew)
        if name.startswith(("pow2", "under")) or name == "outlier":
            # the unclamped scale puts the layer's maximum in [2^14, 2^15): f16's top binade pair
            assert 2.0 ** 14 <= float(np.abs(w).max()) * 2.0 ** ew < 2.0 ** 15, name
    assert {0, X3_EXP_MAX, -X3_EXP_MAX} <= seen


@pytest.mark.parametrize("mod", [CONV, UPS])
@pytest.mark.parametrize("variant", ["default", "outlier", "tiny"])
def test_packed_planes_reconstruct_the_weights(pkg, mod, variant):
    """(hi + lo) 2^-ew against w, elementwise:

        |(hi + lo) 2^-ew - w| <= max(2^-22 |w|, 2^-25 2^-ew)

    2^-22 |w|: hi + lo carry 22 significant bits.  2^-25 2^-ew: half the f16 subnormal quantum
    (2^-24) of the scaled domain, for elements the scale leaves under the normal range.  While
    the exponent is not clamped the layer's maximum times 2^ew is >= 2^14, so the second term
    is <= 2^-39 max|w|, the bound csrc/bf16x3_common.h documents — asserted in that form for
    the outlier layer (one element 2^20 above the rest: every other weight sits under the
    normal range's top by 20 binades).  The 2^-100 layer's exponent is clamped to 60: its
    weights reach the planes as w 2^60 <= 2^-40, under the smallest f16 subnormal, and are
    stored as zeros — an absolute error of at most 2^-100, which the clamped form of the bound
    states and the 2^-39 max|w| form (valid for 2^-45 <= max|w| < 2^75 only) does not."""
    sd = C.make_state_dict(C.V2STAR, seed=171)
    w = sd[mod + ".weight"] if variant == "default" else _weight_variants(sd[mod + ".weight"])[variant]
    h = _handle_with(pkg, sd, **{mod + ".weight": w})
    info, rec = _reconstruct(h, mod, w.shape)
    w64 = w.astype(np.float64)
    err = np.abs(rec - w64)
    bound = np.maximum(2.0 ** -22 * np.abs(w64), 2.0 ** -25 * 2.0 ** -info["ew"])
    print(f"{mod} {variant}: ew {info['ew']} max err {err.max():.3e} "
          f"({(err / np.abs(w64).max()).max():.3e} of max|w|), worst err/bound {(err / bound).max():.3f}")
    assert (err <= bound).all()
    if variant == "tiny":
        assert info["ew"] == X3_EXP_MAX and not rec.any()
    else:
        assert (err <= np.maximum(2.0 ** -22 * np.abs(w64), 2.0 ** -39 * np.abs(w64).max())).all()
        assert rec.any()


# ---- pre-checks of the GPU file's inputs ----------------------------------------------------
def _precheck_regions(ref, L, t0, rf):
    """Coverage, finiteness and a non-zero quiet reference; `err <= bar` below is true by
    construction for finite references (err is the cond inside the bar)."""
    hot, quiet = D.region_masks(L, t0, rf)
    assert D.quiet_reference_ok(ref.ref64[0], quiet), "quiet region: coverage / finite / non-zero"
    for mask in (hot, quiet):
        err, bar, cond, _ = D.region_check(ref.ref32[0], ref.ref64[0], ref.ref32[0], mask,
                                           D.STAGE_RTOL["fp32"])
        assert np.isfinite(err) and err <= bar
    err, bar, _, _ = D.region_check(ref.ref32[1], ref.ref64[1], ref.ref32[1], None,
                                    D.STAGE_RTOL["fp32"])
    assert np.isfinite(err) and err <= bar
    return float(quiet.mean())


@pytest.mark.parametrize("name", [b.name for b in D.SPIKE_BLOCKS])
def test_spike_inputs_oracle_meets_regional_bars(pkg, name):
    blk = D._BLOCKS[name]
    cover = []
    for pos in D.spike_positions(pkg, name):
        for ratio in D.SPIKE_RATIOS + ([D.LIMIT_RATIO] if blk is D.LIMIT_BLOCK else []):
            x, ref, t0, L = D.spike_case(pkg, name, pos, ratio)
            assert float(np.abs(x[0, :, t0]).max()) > 100 * float(np.abs(x[1]).max()) / 8
            cover.append(_precheck_regions(ref, L, t0, blk.rf))
            assert 0 < ref.allowance < np.inf
    print(f"{name}: windows {D.block_windows(pkg, blk)}, RF {blk.rf}, quiet coverage >= {min(cover):.2f}")


@pytest.mark.parametrize("name", [b.name for b in D.OUTLIER_BLOCKS])
def test_outlier_inputs_oracle_meets_componentwise_bar(pkg, name):
    """The reference is finite and non-zero and the sensitivity S is positive everywhere; the
    oracle's `err <= bar` is true by construction (the bar contains 4 * max err)."""
    x, ref = D.outlier_case(pkg, name)
    cond = float(np.abs(ref.ref32 - ref.ref64).max())
    err = np.abs(ref.ref32 - ref.ref64)
    assert np.isfinite(ref.ref64).all() and np.abs(ref.ref64).max() > 0
    assert (err <= D.STAGE_RTOL["fp32"] * ref.sens + 4 * cond).all()
    assert ref.sens.min() > 0


@pytest.mark.parametrize("k", D.EXACT_K)
@pytest.mark.parametrize("under", [False, True])
def test_exact_maximum_inputs(k, under):
    x, ref = D.exact_max_case(k, under)
    m = float(np.abs(x).max())
    assert math.frexp(m) == ((0.5, k + 1) if not under else (1 - 2.0 ** -24, k))
    err, bar, _, _ = D.region_check(ref.ref32, ref.ref64, ref.ref32, None, D.STAGE_RTOL["fp32"])
    assert np.isfinite(err) and err <= bar


@pytest.mark.parametrize("name", ["v1", "v2star"])
def test_logmel_input_oracle_meets_stage_and_regional_bars(name):
    mel = D.logmel_input()
    assert mel.dtype == np.float32 and mel.shape == (2, 80, 48)
    assert (mel[0, :, 16:32] == np.float32(D.LOG_FLOOR)).all() and (mel[1] == np.float32(D.LOG_FLOOR)).all()
    assert D.LOG_FLOOR <= mel.min() and 0.0 < mel.max() < 6.0 and mel[0, :, :16].std() > 1.0
    r64, r32 = D.logmel_refs(name)
    f0, f1 = D.LOGMEL_QUIET
    for tap, rate in D.stage_rates(D.GEN_CONFIGS[name]).items():
        ref, o32 = r64[tap], r32[tap]
        assert np.isfinite(ref).all()
        quiet = np.zeros(ref.shape[-1], bool)
        quiet[f0 * rate:f1 * rate] = True
        assert np.abs(ref[0][..., quiet]).max() > 0
        for b, mask in ((slice(None), None), (0, quiet), (0, ~quiet)):
            err, bar, _, _ = D.region_check(o32[b], ref[b], o32[b], mask, D.STAGE_RTOL["fp32"])
            assert err <= bar, (tap, err, bar)


@pytest.mark.parametrize("name", ["v2star", "c128x2"])
def test_extreme_inputs_oracle_meets_stage_bars(name):
    mel = D.extremes_input()
    assert [float(np.abs(mel[b]).max()) > 0 for b in range(4)] == [True, True, True, False]
    assert np.abs(mel[2]).max() / np.abs(mel[0]).max() > 2.0 ** 78
    for b, n in enumerate(D.EXTREME_LENS):
        assert not mel[b, :, n:].any()
        r64, r32 = D.extremes_refs(name, b)
        for tap in r64:
            assert np.isfinite(r64[tap]).all() and np.isfinite(r32[tap]).all(), (b, tap)
            err, bar, _, _ = D.region_check(r32[tap], r64[tap], r32[tap], None, D.STAGE_RTOL["fp32"])
            assert err <= bar


def test_nan_input_oracle_has_a_finite_far_field():
    """The T = 40 case of the issue has no sample further than 2 RF frames from frame 20 (V1's
    RF bound is 15 frames); the T = 96 case added beside it does, and the oracle is finite
    there and NaN around the frame."""
    rf = D.rf_frames(C.V1)
    assert rf == 15
    for T in (40, 96):
        wav = D.nan_oracle(T, False)
        assert np.isfinite(wav[0]).all() and np.isfinite(wav[2]).all()
        nan = np.isnan(wav[1, 0])
        frames = np.arange(wav.shape[-1]) // 256
        assert nan[frames == D.NAN_FRAME].all()
        far = np.abs(frames - D.NAN_FRAME) > 2 * rf
        assert far.any() == (T == 96)
        assert not nan[far].any()


def test_subnormal_grid_input():
    """Scale exponent 0 (maximum 1.5 * 2^14), every other element an odd multiple of 2^-24 under
    2^-20; the fp32 oracle meets the componentwise fp32-class bar of the GPU test, and the same
    conv on inputs rounded to the grid of a scale one binade lower (2^-23) misses it widely."""
    x, ref = D.subnormal_grid_case()
    blk = D.GRID_BLOCK
    assert math.frexp(float(np.abs(x).max()))[1] == 15
    rest = np.delete(x.astype(np.float64), D.GRID_SPIKE, axis=2) * 2.0 ** 24
    assert (rest == np.round(rest)).all() and (rest % 2 == 1).all() and rest.max() < 16
    far = np.abs(np.arange(D.GRID_L) - D.GRID_SPIKE) > blk.rf
    bar = (3 * 2.0 ** -22 + (blk.channels * 3 + 2) * 2.0 ** -24) * ref.sens[..., far]
    assert (np.abs(ref.ref32 - ref.ref64)[..., far] <= bar).all()
    coarse = np.round(x.astype(np.float64) * 2.0 ** 23) * 2.0 ** -23   # ties to even
    w = D.block_state(blk)["resblocks.0.convs.0.weight"].astype(np.float64)
    y = x + D.N.conv1d(D.N.lrelu(coarse), w, np.zeros(blk.channels), 1, 1)
    assert np.median(np.abs(y - ref.ref64)[..., far] / bar) > 100


# ---- the thin kernels' windows --------------------------------------------------------------
def test_thin_windows_come_from_the_library(pkg):
    """The plan lists a thin launch's halos but not its kernel's window; the spike positions
    of the thin entries take it from hfg_debug_thin_window, so a kernel whose window changes
    moves the spikes with it.  Two full windows fit the input, and the library knows no window
    for a channel count without a thin kernel."""
    lib = pkg.load_library()
    assert lib.hfg_debug_thin_window(64, 0) == 0 and lib.hfg_debug_thin_window(8, 1) == 0
    for blk in D.SPIKE_BLOCKS:
        if blk.j >= 0:
            continue
        (w, halo), = D.block_windows(pkg, blk)
        nwin = lib.hfg_debug_thin_window(blk.channels, 0)
        assert nwin % 16 == 0 and w == nwin - 2 * halo and halo == blk.rf and w >= nwin // 4
        L, pos = D.spike_geometry([(w, halo)])
        assert L > w and pos == {"a": w // 2, "b": w - 1, "c": w - halo}
