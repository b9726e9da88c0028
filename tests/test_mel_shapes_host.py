"""Host side of the mel / resampler shape tests (mel_cases.py): the case tables the GPU tests
iterate reach what they claim to reach, the oracle meets the conditions the DFT bars rest on,
host-only handles accept and refuse what the Python classes will, the resampler's tables and
lengths are the oracle's, its fp32 fma chain leaves room under the output bar, and every mutant
of the float64 references leaves the bar at a listed case (a case set that cannot see such an
error is no coverage).  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import mel_cases as MC
from oracle import mel_torch as M
from oracle import resample_np as R

ALL_DFT = MC.DFT_CONFIGS + [MC.DFT_FORCED]


def _ids(cfgs):
    return [c["name"] for c in cfgs]


def test_case_tables_reach_the_paths():
    """FFT configurations are powers of two, unforced DFT ones are not; between them the tables
    hold win_length < n_fft, a hop that does not divide n_fft, hop >= n_fft / 2, n_mels > 64,
    empty bands, htk / norm=None, f_min > 0, the short Stockham plans, every residue of the
    frame count in two blocks, the bin-tile tail, an odd k trip count and a hop off the
    power-of-two grid on the DFT path."""
    assert all(MC.is_pow2(c["n_fft"]) for c in MC.FFT_CONFIGS)
    assert not any(MC.is_pow2(c["n_fft"]) for c in MC.DFT_CONFIGS)
    assert MC.is_pow2(MC.DFT_FORCED["n_fft"])
    F = MC.FFT_CONFIGS
    assert any(c["win_length"] < c["n_fft"] for c in F)
    assert any(c["n_fft"] % c["hop_length"] for c in F)
    assert any(2 * c["hop_length"] >= c["n_fft"] for c in F)
    assert any(c["hop_length"] == c["n_fft"] for c in F)
    assert any(c["n_mels"] > 64 for c in F)
    assert any(c["mel_scale"] == "htk" and c["norm"] is None for c in F)
    assert any(c["f_min"] > 0 for c in F)
    assert {16, 32, 64, 128} <= {c["n_fft"] for c in F}
    for c in F:
        fpb = MC.fft_fpb(c)
        counts = {MC.frames(c, n) for n in MC.fft_lengths(c)}
        first = {f for f in range(1, fpb + 1) if (f - 1) * c["hop_length"] >= MC.shortest(c)}
        assert first | set(range(fpb + 1, 2 * fpb + 2)) <= counts, c["name"]
        assert {f % fpb for f in counts} == set(range(fpb)), c["name"]
        assert MC.shortest(c) in MC.fft_lengths(c) and MC.shortest(c) + 1 in MC.fft_lengths(c)
        assert all(n > c["n_fft"] // 2 for n in MC.fft_lengths(c))
        assert max(MC.fft_lengths(c)) <= 65 * 512
    for name, n_empty in MC.EMPTY_BANDS.items():
        c = MC.BY_NAME[name]
        fb = M.melscale_fbanks(MC.n_bins(c), c["f_min"], c["f_max"], c["n_mels"],
                               c["sample_rate"], c["norm"], c["mel_scale"])
        assert int((fb == 0).all(0).sum()) == n_empty
    D = MC.DFT_CONFIGS
    assert any(MC.n_bins(c) == 201 for c in D)                      # bins_pad 224: seven tiles
    assert any(MC.n_bins(c) % 32 == 0 for c in D)                   # n_bins = bins_pad
    assert any((c["n_fft"] // 2) % 2 for c in D)                    # odd trip count of the k loop
    assert any(not MC.is_pow2(c["hop_length"]) for c in D)          # the skewed LDS layout
    for c in ALL_DFT:
        counts = {MC.frames(c, n) for n in MC.dft_lengths(c)}
        assert set(MC.DFT_FRAME_COUNTS) <= counts
        assert any(n % c["hop_length"] == c["hop_length"] - 1 for n in MC.dft_lengths(c))
        assert max(MC.dft_lengths(c)) <= 65 * 512


def test_reference_restatements_are_the_oracles():
    """mel_variant / resample_variant, the hooks the mutants hang on, are bitwise log_mel64 /
    resample when nothing is mutated."""
    for c in MC.FFT_CONFIGS + ALL_DFT:
        for n in (MC.lengths(c)[0], MC.lengths(c)[-1]):
            wav, ref = MC.mel_ref(c["name"], n)
            assert torch.equal(MC.mel_variant(wav, c), ref), (c["name"], n)
    for (orig, new) in MC.RESAMPLE_PAIRS:
        n = MC.resample_lengths(orig, new)[-1]
        x = MC.resample_rows(n, orig)
        assert np.array_equal(MC.resample_variant(x, orig, new), R.resample(x, orig, new))


@pytest.mark.parametrize("cfg", ALL_DFT, ids=_ids(ALL_DFT))
def test_dft_inputs_have_no_quiet_band(cfg, evidence):
    """Every band of every DFT case lies within 6 decades of its item's maximum on the float64
    oracle, so the 5e-4 bar covers all of them (the fp32 oracle's 2e-2 bar on quieter bands is
    not carried over: there two fp32 methods differ by that much from float64 themselves).
    Prints the reference's own fp32-vs-float64 difference, the room the DFT bars have to leave,
    and holds it under a tenth of the tighter bar: on these inputs the bars measure the device,
    not the reference's rounding."""
    worst_range, worst32 = 0.0, 0.0
    for n in MC.dft_lengths(cfg):
        wav, ref = MC.mel_ref(cfg["name"], n)
        for b in range(3):
            worst_range = max(worst_range, float(ref[b].max() - ref[b].min()))
            assert bool(MC.dft_masks(ref[b])[1].all()), (cfg["name"], n, b)
        worst32 = max(worst32, float((M.log_mel(wav, cfg).double() - ref).abs().max()))
    evidence(f"{cfg['name']}: widest item range {worst_range:.2f} decades (limit {MC.DFT_DECADES}); "
             f"fp32 oracle vs float64 oracle {worst32:.2e} (DFT bars {MC.DFT_BAR_STRONG:g} / {MC.DFT_BAR:g})")
    assert worst32 <= 0.1 * MC.DFT_BAR_STRONG


def test_host_handles_accept_and_refuse(pkg):
    """Host-only handles (device -1) take every configuration of the tables; the FFT ones report
    the token 256-byte workspace, the DFT ones (forced: under the MEL_DFT override, see the GPU
    test) 4 B frames n_bins; the refusal cases return -22."""
    lib = pkg.load_library()
    for c in MC.FFT_CONFIGS + MC.DFT_CONFIGS:
        h = ctypes.c_void_p()
        assert lib.hfg_mel_create(ctypes.byref(MC.c_config(pkg, c)), -1, ctypes.byref(h)) == 0, c["name"]
        for n in MC.lengths(c):
            assert lib.hfg_mel_frames(h, n) == MC.frames(c, n)
            want = 256 if c in MC.FFT_CONFIGS else MC.dft_workspace_bytes(c, 3, n)
            assert lib.hfg_mel_workspace_bytes(h, 3, n) == want, (c["name"], n)
        # N = n_fft / 2 (and anything else) on a host-only handle
        assert lib.hfg_mel_forward(h, None, 3, c["n_fft"] // 2, None, None, 0, None) == -22
        lib.hfg_mel_destroy(h)
    for c in MC.REFUSED_CONFIGS:
        h = ctypes.c_void_p()
        assert lib.hfg_mel_create(ctypes.byref(MC.c_config(pkg, c)), -1, ctypes.byref(h)) == -22, c["name"]
        assert not h.value


def test_forced_dft_workspace(pkg, sched):
    lib = pkg.load_library()
    c = MC.DFT_FORCED
    sched("MEL_DFT", 1)
    h = ctypes.c_void_p()
    assert lib.hfg_mel_create(ctypes.byref(MC.c_config(pkg, c)), -1, ctypes.byref(h)) == 0
    n = MC.dft_lengths(c)[-1]
    assert lib.hfg_mel_workspace_bytes(h, 3, n) == MC.dft_workspace_bytes(c, 3, n)
    lib.hfg_mel_destroy(h)


PAIRS = list(MC.RESAMPLE_PAIRS)
PAIR_IDS = [f"{o}-{n}" for o, n in PAIRS]


@pytest.mark.parametrize("orig,new", PAIRS, ids=PAIR_IDS)
def test_resample_tables_and_lengths(pkg, orig, new):
    """hfg_resample_kernel within 1e-7 of R.sinc_kernel, the (phases, stride, klen) the issue
    lists, hfg_resample_out_len the oracle's length at every listed n, and which of the output
    block edges 255 .. 513 some input length hits exactly."""
    lib = pkg.load_library()
    w, p, k = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    assert lib.hfg_resample_kernel(orig, new, 6, 0.99, None, ctypes.byref(w), ctypes.byref(p),
                                   ctypes.byref(k)) == 0
    ref, width = R.sinc_kernel(orig, new)
    assert (p.value, MC.reduced(orig, new)[0], k.value) == MC.RESAMPLE_PAIRS[(orig, new)]
    assert (w.value, p.value, k.value) == (width, ref.shape[0], ref.shape[1])
    got = np.zeros(ref.shape, np.float32)
    assert lib.hfg_resample_kernel(orig, new, 6, 0.99,
                                   got.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                   None, None, None) == 0
    assert np.abs(got - ref).max() <= MC.KERNEL_BAR
    h = ctypes.c_void_p()
    assert lib.hfg_resample_create(orig, new, 6, 0.99, -1, ctypes.byref(h)) == 0
    x1 = np.zeros((1, 1), np.float32)
    for n in MC.resample_lengths(orig, new):
        want = R.resample(np.zeros((1, n), np.float32), orig, new).shape[-1]
        assert lib.hfg_resample_out_len(h, n) == want == MC.out_len(orig, new, n), n
    lib.hfg_resample_destroy(h)
    assert R.resample(x1, orig, new).shape[-1] >= 1
    assert MC.out_hit(orig, new) == MC.OUT_HIT[(orig, new)]
    ls = MC.resample_lengths(orig, new)
    stride = MC.reduced(orig, new)[0]
    assert {1, 2, width, width + 1, stride, stride + 1} <= set(ls) and min(ls) == 1
    assert any(n < width for n in ls)          # an input shorter than the filter half-width
    assert {MC.out_len(orig, new, n) for n in ls} >= set(MC.OUT_HIT[(orig, new)])


@pytest.mark.parametrize("orig,new", PAIRS, ids=PAIR_IDS)
def test_resample_fma_chain_under_the_bar(orig, new, evidence):
    """The kernel's arithmetic emulated on the CPU (mel_cases.fma_chain: one sequential fp32 fma
    chain over klen taps per output) stays under 2e-6 x max|x| of the float64 oracle at every
    pair, klen 15 to 694: the bar has room for a correct kernel."""
    worst = 0.0
    for n in MC.resample_lengths(orig, new)[-2:]:
        x = MC.resample_rows(n, orig)
        err = float(np.abs(MC.fma_chain(x, orig, new).astype(np.float64) -
                           R.resample(x, orig, new)).max())
        worst = max(worst, err / float(np.abs(x).max()))
    evidence(f"resample {orig}->{new}: fp32 fma chain vs float64 oracle {worst:.2e} x max|x| "
             f"(bar {MC.RESAMPLE_BAR:g}, margin x{MC.RESAMPLE_BAR / max(worst, 1e-30):.1f})")
    assert worst <= MC.RESAMPLE_BAR


def _mel_bar_broken(cfg, ref, mut):
    """Would a device output equal to `mut` fail the configuration's bars against `ref`?"""
    e = (mut - ref).abs()
    if cfg in MC.FFT_CONFIGS:
        return float(e.max()) > MC.FFT_BAR
    return any(float(e[b][MC.dft_masks(ref[b])[1]].max()) > MC.DFT_BAR for b in range(ref.shape[0]))


@pytest.mark.parametrize("mutant", list(MC.MEL_MUTANTS))
def test_mel_mutants_leave_the_bar(mutant, evidence):
    """Each mutant of the float64 mel reference (reflect pad -> zero pad; the last frame of a
    partial block dropped; a short window at offset 0 instead of centred) leaves the bar at one
    or more lengths of EVERY configuration it applies to, on both paths."""
    seen = []
    for c in MC.FFT_CONFIGS + ALL_DFT:
        if not MC.mel_mutant_applies(c, mutant):
            continue
        caught = []
        for n in MC.lengths(c):
            wav, ref = MC.mel_ref(c["name"], n)
            if _mel_bar_broken(c, ref, MC.mel_mutant(wav, c, mutant)):
                caught.append(n)
        assert caught, (mutant, c["name"])
        seen.append(f"{c['name']} {len(caught)}/{len(MC.lengths(c))}")
    assert seen
    evidence(f"mel mutant {mutant}: lengths that catch it: " + ", ".join(seen))


@pytest.mark.parametrize("mutant", list(MC.RESAMPLE_MUTANTS))
def test_resample_mutants_leave_the_bar(mutant, evidence):
    """Each mutant of the float64 resample reference (phase index + 1; the left zero pad one
    sample short) leaves 2e-6 x max|x| at one or more lengths of every pair, on the random rows
    and on the impulses."""
    seen = []
    for (orig, new) in PAIRS:
        caught_rows, caught_imp = [], []
        for n in MC.resample_lengths(orig, new):
            for x, caught in ((MC.resample_rows(n, orig), caught_rows), (MC.impulses(n), caught_imp)):
                ref = R.resample(x, orig, new)
                mut = MC.resample_variant(x, orig, new, **MC.RESAMPLE_MUTANTS[mutant])
                if float(np.abs(mut - ref).max()) > MC.RESAMPLE_BAR * float(np.abs(x).max()):
                    caught.append(n)
        assert caught_rows and caught_imp, (mutant, orig, new)
        seen.append(f"{orig}->{new} {len(caught_rows)}+{len(caught_imp)}")
    evidence(f"resample mutant {mutant}: lengths that catch it (rows+impulses): " + ", ".join(seen))
