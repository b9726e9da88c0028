"""Tap geometry at the planner's limits on the GPU (tests/tap_cases.py; the host side, which pins
every case to its limit and shows what the probes resolve: test_taps_host.py).

1. Standalone ResBlock / ResBlock2 / MRF probes whose kernel size, dilations or conv count sit
   on a limit of the whole-block, thin or layer kernels (or one step to either side), at every
   length class of every launch geometry of the handle, in all four precisions, against float64.
2. One-stage generators whose upsampler reads the mel itself, on weights with every tap loud and
   distinct: the (u, k) pairs of tap_cases.UPS_CASES at lengths on both sides of every tile
   edge, full batches on the ups.0 tap and ragged batches on the wav.

No tolerance is introduced: block and stage tensors under the stage bar of test_gpu_stages.py
(cond = 0: the probes are exact, the expected error is 0), wavs under the project's 1e-4.  Every
run asserts from the launch profile that the launch the case names ran."""
import numpy as np
import pytest
import torch

import seam_cases as S
import tap_cases as T
from test_gpu_seams import _first_wrong, _launches, _profiled, _t
from width_cases import bf16x3_instances, fp32_instances, ups_frames_launches

pytestmark = pytest.mark.gpu
CASE_KNOBS = [(c.name, i) for c in T.CASES for i in range(len(c.knob_sets))]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _kt32(k):
    return k if k in (2, 3, 5, 7, 11) else 0


def _check_launch(case, knobs, precision, summary):
    """The forward ran the launch the case (under these knobs) exists for: seam_cases'
    _check_kernels, extended with the fp32 layer kernel inside a split-precision handle and
    with the tap-count instance of every layer launch."""
    names = sorted(summary)
    whole, whole2 = _launches(summary, "resblock_bf16x3<"), _launches(summary, "resblock2_bf16x3<")
    thin, thin_m = _launches(summary, "mrf_thin<"), _launches(summary, "mrf_thin_mfma<")
    layer, layer32 = _launches(summary, "conv1d_bf16x3<"), _launches(summary, "conv1d_mfma_f32<")
    convs = T.all_convs(case.blk)
    k = case.blk.kernels[0]
    if case.launch in ("thin", "thin_mfma"):
        mfma = case.launch == "thin_mfma" and precision != "fp32"
        assert (thin, thin_m, layer, layer32) == ((0, 1, 0, 0) if mfma else (1, 0, 0, 0)), names
        return
    if precision == "fp32":
        assert layer32 == len(convs) and not (whole + whole2 + layer + thin + thin_m), names
        assert {(kt, tile, ck) for kt, tile, ck, _ in fp32_instances(summary)} == \
            {(_kt32(k), tile, ck) for _, tile, ck, _ in case.pin32[-1]}, names
        return
    if case.launch == "layer" or knobs.get("FUSED_RB") == 0:
        n32 = len(case.fp32_convs)
        # a conv past the split kernel's reach runs conv1d_mfma_f32 and no conv1d_bf16x3
        assert (layer, layer32) == (len(convs) - n32, n32) and not (whole + whole2 + thin + thin_m), names
        small = knobs.get("SMALL_TILE")
        want = {(k if k in (3, 5, 7, 11) else 0, st if small and st >= 0 else tile, False)
                for prec, tile, _, st in case.pin16[-1] if prec == 1}
        if small is not None or case.launch == "layer" and not any(st >= 0 for *_, st in case.pin16[-1]):
            assert bf16x3_instances(summary) == want, (names, want)
        assert {(kt, tile, ck) for kt, tile, ck, _ in fp32_instances(summary)} == \
            {(_kt32(k), tile, ck) for prec, tile, ck, _ in case.pin16[-1] if prec == 0}, names
    elif case.launch == "rb2":
        assert (whole2, whole, layer, layer32) == (1, 0, 0, 0), names
    else:
        split = case.launch == "split" and knobs.get("RB_SPLIT", 1)
        assert (whole, whole2, layer, layer32) == (2 if split else 1, 0, 0, 0), names


# ----------------------------------------------------------------------------------------
# 1. ResBlock / ResBlock2 / MRF probes on the tap axis
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ks", CASE_KNOBS, ids=[f"{n}-{k}" for n, k in CASE_KNOBS])
def test_tap_limit_probe_at_every_length_class(pkg, dev, sched, evidence, name, ks):
    """The case's module on its probe weights, x [2, C, L] for every length class of every
    launch geometry of the handle, under the case's knob set ks, against float64.  fp32
    ignores the knobs and runs under the first set only.  Every value is an integer < 2^16 in
    every format (test_taps_host.py): the expected error is exactly 0; the asserted bar is the
    stage bar (TapCase.rtol: the 16-conv list holds bf16x3 to f16x3's)."""
    case = T.BY_NAME[name]
    blk = case.blk
    ws, Ls = S.block_windows(pkg, blk), S.block_lengths(pkg, blk)   # before any override
    knobs = case.knob_sets[ks]
    for k, v in knobs.items():
        sched(k, v)
    worst = {}
    for precision in (S.PRECISIONS if ks == 0 else S.SPLIT_PRECISIONS):
        mod = S.make_module(pkg, blk, precision, dev, T.tap_state(name))
        for L in Ls:
            x, ref = T.tap_ref(pkg, name, L)
            if L == Ls[-1]:
                y, summary = _profiled(mod._handle_for(dev), lambda: mod(_t(x, dev)))
                _check_launch(case, knobs, precision, summary)
            else:
                with torch.no_grad():
                    y = mod(_t(x, dev))
            got = y.cpu().numpy().astype(np.float64)
            assert got.shape == ref.shape
            err = float(np.abs(got - ref).max())
            bar = case.rtol(precision) * max(1.0, float(np.abs(ref).max()))
            print(f"{precision} L {L}: err {err:.3g} bar {bar:.3g}")
            worst[precision] = max(worst.get(precision, 0.0), err)
            assert err <= bar, (case.why, precision, knobs, L, _first_wrong(got, ref, bar, ws, L))
    evidence(f"{knobs or 'default schedule'}, {len(Ls)} lengths: max err " +
             ", ".join(f"{p} {e:.3g}" for p, e in worst.items()))


# ----------------------------------------------------------------------------------------
# 2. upsampler (u, k) pairs
# ----------------------------------------------------------------------------------------
# (case, UPS_FRAMES): 1 keeps grids this small on the polyphase kernel, 2 runs the output-frame
# kernel wherever the plan packs it (k = 2u) and the batch width is a multiple of 4
UPS_MODES = [(c.name, m) for c in T.UPS_CASES for m in ((1, 2) if c.frames else (1,))]
UPS_IDS = [f"{n}-frames{m}" for n, m in UPS_MODES]


def _ups_gen(pkg, name, precision, dev):
    """(the probe weights are bf16-exact, test_taps_host.py: bf16w computes the same model)"""
    case = T.UPS_BY_NAME[name]
    gen = pkg.HiFiGANGenerator(**case.cfg.kwargs(), precision=precision).eval()
    gen.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in T.ups_state(name).items()})
    return gen.to(dev)


def _check_ups_kernel(case, precision, frames, summary):
    """ups.0 ran the kernel the case names: the output-frame kernel on the plan's
    configuration, else the polyphase kernel of the plan's precision on its tile (or the small
    tile) and its tap-count instance: KT = 2 compile-time, any other runtime."""
    names = sorted(summary)
    assert ups_frames_launches(summary) == ({case.pin16[4][0]: 1} if frames else {}), names
    split = {i for i in bf16x3_instances(summary) if i[2]}
    f32 = {i for i in fp32_instances(summary) if i[3]}
    if frames:
        assert not split and not f32, names
    elif precision != "fp32" and case.pin16[0] == 1:
        assert len(split) == 1 and not f32, names
        (kt, tile, _), = split
        assert kt == (2 if case.KT == 2 else 0) and tile in (case.pin16[1], case.pin16[3]), names
    else:   # the fp32 precision, or KT = 17 inside a split-precision handle
        pin = case.pin32 if precision == "fp32" else case.pin16
        assert not split and f32 == {(_kt32(case.KT), pin[1], pin[2], True)}, names


@pytest.mark.parametrize("name,mode", UPS_MODES, ids=UPS_IDS)
def test_ups_probe_full_batches(pkg, dev, sched, evidence, name, mode):
    """forward_with_stages on mel [2, c0, L], L in {1 .. 5} and on both sides of every tile
    edge: the ups.0 tap against float64 under the stage bar (the expected error is 0; the
    signed case: 0.1f against 0.1), the wav under 1e-4."""
    case = T.UPS_BY_NAME[name]
    Ls = T.ups_lengths(pkg, name)
    sched("UPS_FRAMES", mode)
    worst = {}
    for precision in (S.PRECISIONS if mode == 1 else S.SPLIT_PRECISIONS):
        gen = _ups_gen(pkg, name, precision, dev)
        h = gen.hip_handle(dev)
        for L in Ls:
            mel = _t(T.ups_mel(name, L), dev)
            (wav, stages), summary = _profiled(h, lambda: gen.forward_with_stages(mel))
            _check_ups_kernel(case, precision, mode == 2 and L % 4 == 0, summary)
            r = T.ups_refs(name, L)
            got = stages["ups.0"].cpu().numpy().astype(np.float64)
            assert got.shape == r["ups.0"].shape == (2, case.c0 // 2, case.out_len(L))
            err = float(np.abs(got - r["ups.0"]).max())
            bar = S.RTOL[precision] * max(1.0, float(np.abs(r["ups.0"]).max()))
            print(f"{precision} L {L}: err {err:.3g} bar {bar:.3g}")
            worst[precision] = max(worst.get(precision, 0.0), err)
            bad = np.flatnonzero((np.abs(got - r["ups.0"]) > bar).any(axis=(0, 1)))
            assert err <= bar, (case.why, precision, L, f"wrong output samples {bad[:8]} of {got.shape[-1]}")
            assert float(np.abs(wav.cpu().numpy() - r["wav"]).max()) < S.ATOL, (precision, L)
    evidence(f"UPS_FRAMES {mode}, L in {Ls}: max ups.0 err " +
             ", ".join(f"{p} {e:.3g}" for p, e in worst.items()))


def _ragged(name, T_, lens):
    mel = np.array(T.ups_mel(name, T_, len(lens)))
    for b, n in enumerate(lens):
        mel[b, :, n:] = -77.0
    return mel


@pytest.mark.parametrize("name,mode", UPS_MODES, ids=UPS_IDS)
def test_ups_probe_ragged_batches(pkg, dev, sched, evidence, name, mode):
    """Item ends at each position of a frame quad and on both sides of every tile edge, -77 in
    the mel's padding: each item bitwise its solo run, zero past its output length, its solo
    wav within 1e-4 of its float64 wav."""
    case = T.UPS_BY_NAME[name]
    sched("UPS_FRAMES", mode)
    worst = {}
    batches = T.ups_ragged_batches(pkg, name)
    for precision in (S.PRECISIONS if mode == 1 else S.SPLIT_PRECISIONS):
        gen = _ups_gen(pkg, name, precision, dev)
        h = gen.hip_handle(dev)
        for T_, lens in batches:
            mel = _ragged(name, T_, lens)
            out, summary = _profiled(h, lambda: gen(_t(mel, dev), lengths=lens))
            _check_ups_kernel(case, precision, mode == 2, summary)
            with torch.no_grad():
                for b, n in enumerate(lens):
                    solo = gen(_t(mel[b:b + 1, :, :n], dev))
                    m = case.out_len(n)
                    assert solo.shape[-1] == m == gen.output_length(n)
                    assert torch.equal(out[b:b + 1, :, :m], solo), (precision, T_, lens, b)
                    assert not out[b, :, m:].any(), (precision, T_, lens, b)
                    ref = T.ups_refs(name, T_, len(lens), b, n)["wav"]
                    err = float(np.abs(solo.cpu().numpy() - ref).max())
                    worst[precision] = max(worst.get(precision, 0.0), err)
                    assert err < S.ATOL, (precision, T_, lens, b, err)
    evidence(f"UPS_FRAMES {mode}, batches {batches}: max wav err " +
             ", ".join(f"{p} {e:.2e}" for p, e in worst.items()))


@pytest.mark.parametrize("name,mode", [("u8_k16", 2), ("u8_k16", 1), ("u4_k9", 1), ("u2_k34", 1)])
def test_ups_probe_ignores_stale_buffers(pkg, dev, sched, name, mode):
    """A ragged batch on a workspace and a wav whose every byte is 0xFF (NaN bit patterns), as
    test_gpu_ups_staging.py::test_padding_rows_hold_no_data: each item bitwise its solo run and
    zero past its length."""
    case = T.UPS_BY_NAME[name]
    sched("UPS_FRAMES", mode)
    T_, lens = 12, [12, 7, 10, 1]
    mel = _t(_ragged(name, T_, lens), dev)
    ln = torch.tensor(lens, dtype=torch.int32, device=dev)
    for precision in S.PRECISIONS:
        gen = _ups_gen(pkg, name, precision, dev)
        h = gen.hip_handle(dev)
        out_len, nbytes = h.out_len(T_), h.workspace_bytes(len(lens), T_)
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
        wav = torch.full((len(lens) * out_len * 4,), 0xFF, dtype=torch.uint8, device=dev).view(torch.float32)
        wav = wav.view(len(lens), 1, out_len)
        torch.cuda.synchronize()

        def run():
            h.forward_ex(mel.data_ptr(), len(lens), T_, wav.data_ptr(), out_len, ws.data_ptr(), nbytes,
                         torch.cuda.current_stream(dev).cuda_stream, lengths_ptr=ln.data_ptr())
            return wav

        _, summary = _profiled(h, run)
        _check_ups_kernel(case, precision, mode == 2 and case.frames and precision != "fp32", summary)
        for b, n in enumerate(lens):
            with torch.no_grad():
                solo = gen(mel[b:b + 1, :, :n].contiguous())
            m = case.out_len(n)
            assert torch.equal(wav[b:b + 1, :, :m], solo), (precision, b)
            assert not wav[b, :, m:].any(), (precision, b)
