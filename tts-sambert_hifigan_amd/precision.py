"""Documented accuracy of the arithmetic modes, by weight scale.

``f16x3`` (the default) scales every operand by a power of two into the f16 range and splits
it into f16 halves hi + lo (22 significant bits); hi*hi + hi*lo + lo*hi are summed in fp32 on
the f16 matrix cores (csrc/bf16x3_common.h).  Its products miss the exact ones by ~2^-21
relative, below the fp32 rounding the reference itself makes, so it meets the bars of exact
fp32 on every golden fixture — the x4 "loud" ones included — at the bf16x3 rate.  A value the
scaling leaves under the f16 normal range keeps an absolute error <= 2^-39 of its tensor's
(weights: layer's) largest magnitude while the scale exponent is not clamped (+-60), i.e. for
a largest magnitude in [2^-45, 2^75); a smaller tensor may be stored as zeros, a larger one
overflows f16 (tests/test_dynamic_range_host.py, tests/test_gpu_dynamic_range.py).

``bf16x3`` splits into bf16 halves without scaling: ~16-bit-mantissa products (stage error
<= 2.5e-5 relative at every scale, tests/test_gpu_stages.py).  That meets the north star's
1e-4 on the wav for weights up to twice PyTorch's default-init scale.  At x4 scale the
pre-tanh values of the V2* fixture reach ~5e3 and tanh is 99.8 % saturated; the few samples
at its zero crossings move by up to 0.084 (tests/tools/diag_precision.py: no single stage
dominates, every stage adds its 1e-5-relative share).  That is above the conditioning bar
exact fp32 meets there, max(1e-4, 50 x |ref_fp32 - ref_fp64|) = 0.0675 (fp32: 2.0e-3).

``BF16X3_SCALE_LIMITS[s]``: the limit asserted by tests/test_gpu_stages.py::
test_bf16x3_scale_limits on the golden fixtures of weight scale ``s``:
``max_abs`` = largest |wav - reference wav| allowed, ``within_1e-4`` = smallest
fraction of samples within 1e-4.  ``MEASURED`` = what the MI355X runs gave.
"""

BF16X3_SCALE_LIMITS = {
    1.0: {"max_abs": 1e-4, "within_1e-4": 1.0},
    2.0: {"max_abs": 1e-4, "within_1e-4": 1.0},
    4.0: {"max_abs": 0.15, "within_1e-4": 0.995},
}

MEASURED = {
    "f16x3": {1.0: "2-5e-8 (g1-g5, g7, g8)", 2.0: "1.2e-6 (g6)",
              4.0: "g9 0 (saturated); g10 2.1e-3 (bar 6.75e-2, fp32 2.0e-3); per-stage <= 2.5e-6 "
                   "of the stage's max |ref| on all 10 fixtures"},
    "bf16x3": {1.0: "<= 9e-8 (g1-g5, g7, g8)", 2.0: "1.3e-5 (g6)",
               4.0: "g9 0 (saturated); g10 0.084, 99.83% within 1e-4"},
    "fp32": {1.0: "<= 6e-8", 2.0: "1.4e-6 (g6)", 4.0: "g9 0; g10 2.0e-3 (reference fp32 vs fp64: 1.35e-3)"},
    # f16x3, tests/test_gpu_dynamic_range.py (evidence lines of the MI355X run): one column of
    # a standalone block's input times R; max|hip - ref64| / max(1, max|ref64|) over the quiet
    # columns (further than the receptive-field radius from the spike) and the hot ones; worst
    # of the three window positions and of the whole-block / layer-per-launch schedules.  No
    # underflow allowance is granted at R <= 2^16 (bar: 4e-6); the allowance at 2^30 is
    # 2 * 2^-39 * max|operand| * max_row sum|w| summed over the block's convs.
    "dynamic_range": {
        "resblock_bf16x3 (C = 128 / 64 / 32, k = 3 / 7 / 11)": {
            "2^10": "quiet <= 1.7e-7, hot <= 1.1e-7", "2^16": "quiet <= 1.8e-7, hot <= 1.4e-7",
            "2^30": "C = 64 k = 3: quiet 2.4e-3 absolute (1.1e-3 relative; layers 2.5e-3) against "
                    "an allowance of 1.27e-1; hot 4.8e-8 (bf16x3, unscaled: quiet 1.8e-6); spike on "
                    "a window's last column 2.4e-3 against 1.46e-1, on the next window's first "
                    "halo column 2.7e-3 against 1.59e-1"},
        "resblock2_bf16x3 (C = 64, k = 3 / 7)": {
            "2^10": "quiet <= 2.4e-7, hot <= 1.3e-7", "2^16": "quiet <= 2.4e-7, hot <= 8.8e-8"},
        "mrf_thin_mfma (C = 16)": {
            "2^10": "quiet 1.1e-7, hot 8.9e-8", "2^16": "quiet 1.0e-7, hot 5.9e-8"},
        "mrf_thin (C = 8, fp32 VALU)": {
            "2^10": "quiet 8.8e-8, hot 4.4e-8", "2^16": "quiet 8.8e-8, hot 7.9e-8"},
    },
}


def note(precision: str) -> str:
    """One-line statement of the mode's accuracy, for the bench line and docs."""
    if precision == "fp32":
        return ("exact fp32 products: wav within 1e-4 of the reference at default and x2 weight "
                "scale; at x4 within 50x the reference's own fp32-vs-fp64 difference")
    if precision == "f16x3":
        return ("f16x3: products within ~2^-21 relative of exact (fp32-class): every golden "
                "fixture within the exact-fp32 bars, x4 weights included (tests/test_gpu_stages.py)")
    if precision == "bf16x3":
        return ("bf16x3 scale limit (tested, precision.py): wav within 1e-4 of the reference for "
                "weights up to x2 default-init scale (measured 1.3e-5); at x4 (pre-tanh ~5e3) max "
                "0.084 at tanh zero crossings, 99.8% of samples within 1e-4 -- use f16x3 there")
    return "bf16-rounded weights: a different model, within 1e-4 of the oracle on those weights"


def dtype_note(precision: str) -> str:
    """What the bench line's ``dtype`` means."""
    if precision == "fp32":
        return "fp32 operands on the fp32 MFMA (exact products). " + note(precision)
    if precision == "f16x3":
        return ("fp32 in/out and fp32 accumulation; every fp32 operand scaled by a power of two "
                "(per tensor and batch item for activations, per layer for weights) and split "
                "into f16 hi + lo, products hi*hi + hi*lo + lo*hi on the f16 MFMA (the "
                "upsamplers too). " + note(precision))
    if precision == "bf16x3":
        return ("fp32 in/out and fp32 accumulation; every fp32 operand split into bf16 hi + lo, "
                "products hi*hi + hi*lo + lo*hi on the bf16 MFMA. " + note(precision))
    return ("bf16-rounded weights (f16 halves after scaling, lo = 0), activations split into "
            "f16 hi + lo: hi*hi + hi*lo on the f16 MFMA. " + note(precision))
