"""Window seams and sequence ends on the GPU (tests/seam_cases.py; the host side, which fixes
the set of cases and shows what the probes resolve: test_seams_host.py).

The whole-ResBlock kernels (whole and split), resblock2_bf16x3, the thin whole-MRF kernels, the
layer path and the fused conv_post launch on probe weights whose outermost tap reach is as loud
as any other path, at every length class of every launch geometry of the handle, against the
float64 restatement.  No tolerance is introduced: ResBlock / MRF tensors under the stage bar of
test_gpu_stages.py (cond = 0: the probes are exact in fp32), wavs under the project's 1e-4."""
import numpy as np
import pytest
import torch

import seam_cases as S
from oracle import hifigan_np64 as N
from width_cases import bf16_rounded, bf16x3_instances

pytestmark = pytest.mark.gpu
CASE_KNOBS = [(c.name, i) for c in S.CASES for i in range(len(S.knob_sets(c)))]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def _profiled(h, fn):
    h.profile_reset()
    h.set_profiling(True)
    with torch.no_grad():
        out = fn()
    torch.cuda.synchronize()
    h.set_profiling(False)
    return out, h.profile_summary()


def _first_wrong(got, ref, bar, ws, L):
    """Where a failing tensor first leaves its bar: column, distance to the nearest seam / end."""
    bad = np.flatnonzero((np.abs(got - ref) > bar).any(axis=(0, 1)))
    if not bad.size:
        return "within the bar"
    d, what = S.seam_distance([w for w in ws if w.windowed] or ws, int(bad[0]), L)
    return (f"first wrong column {bad[0]} of {L} ({bad.size} wrong, last {bad[-1]}): {d} from the "
            f"{what}; max err {np.abs(got - ref).max():.3g}")


def _launches(summary, prefix):
    return sum(v["launches"] for k, v in summary.items() if k.startswith(prefix))


def _check_kernels(case, knobs, precision, summary):
    """The forward ran the launch the case (under these knobs) exists for."""
    names = sorted(summary)
    whole = _launches(summary, "resblock_bf16x3<")
    whole2 = _launches(summary, "resblock2_bf16x3<")
    thin, thin_m = _launches(summary, "mrf_thin<"), _launches(summary, "mrf_thin_mfma<")
    layer = _launches(summary, "conv1d_bf16x3<")
    n_conv = len(S.case_convs(case.blk, max(case.blk.j, 0)))
    if case.launch in ("thin", "thin_mfma"):
        mfma = case.launch == "thin_mfma" and precision != "fp32"
        assert (thin, thin_m) == ((0, 1) if mfma else (1, 0)), names
        return
    if precision == "fp32":
        assert _launches(summary, "conv1d_mfma_f32<") == n_conv and not (whole + whole2 + layer), names
        return
    if case.launch == "layer" or knobs.get("FUSED_RB") == 0:
        assert layer == n_conv and not (whole + whole2), names
        if "SMALL_TILE" in knobs:
            assert all((t == 4) == bool(knobs["SMALL_TILE"]) for _, t, _ in bf16x3_instances(summary)), names
    elif case.launch == "rb2":
        assert (whole2, whole, layer) == (1, 0, 0), names
    else:
        split = case.launch == "split" and knobs.get("RB_SPLIT", 1)
        assert (whole, whole2, layer) == (2 if split else 1, 0, 0), names


# ----------------------------------------------------------------------------------------
# 1. standalone ResBlock, ResBlock2 and MRF probes at every length class
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ks", CASE_KNOBS, ids=[f"{n}-{k}" for n, k in CASE_KNOBS])
def test_standalone_probe_at_every_length_class(pkg, dev, sched, evidence, name, ks):
    """gen.mrfs[i].resblocks[j](x) / ResBlock2 / mrf(x) (hfg_resblock_forward / hfg_mrf_forward)
    on the probe weights, x [2, C, L] for every length class of every launch geometry of the
    handle, under the case's knob set ks, against float64.  fp32 ignores the knobs and runs
    under the first set only.  The ResBlock probes are integers < 2^16 in every format: the
    expected error is exactly 0; the asserted bar is the stage bar."""
    case = S.BY_NAME[name]
    ws, Ls = S.windows(pkg, name), S.lengths(pkg, name)   # the default schedule's, before any override
    knobs = S.knob_sets(case)[ks]
    for k, v in knobs.items():
        sched(k, v)
    worst = {}
    for precision in (S.PRECISIONS if ks == 0 else S.SPLIT_PRECISIONS):
        mod = S.make_module(pkg, case.blk, precision, dev)
        for L in Ls:
            x, ref = S.probe_ref(name, L)
            if L == Ls[-1]:
                y, summary = _profiled(mod._handle_for(dev), lambda: mod(_t(x, dev)))
                _check_kernels(case, knobs, precision, summary)
            else:
                with torch.no_grad():
                    y = mod(_t(x, dev))
            got = y.cpu().numpy().astype(np.float64)
            assert got.shape == ref.shape
            err = float(np.abs(got - ref).max())
            bar = max(S.RTOL[precision] * max(1.0, float(np.abs(ref).max())), 0.0)
            print(f"{precision} L {L}: err {err:.3g} bar {bar:.3g}")
            worst[precision] = max(worst.get(precision, 0.0), err)
            assert err <= bar, (precision, knobs, L, _first_wrong(got, ref, bar, ws, L))
    evidence(f"{knobs or 'default schedule'}, {len(Ls)} lengths: max err " +
             ", ".join(f"{p} {e:.3g}" for p, e in worst.items()))


# ----------------------------------------------------------------------------------------
# 2. / 4. Generators with a probe tail: ragged batches, stale buffers
# ----------------------------------------------------------------------------------------
def _gen_sd(name, precision):
    sd = S.gen_state(name)
    return bf16_rounded(sd) if precision == "bf16w" else sd


_WAV64 = {}


def _wav64(name, precision, b, n):
    """float64 wav of item b alone on its first n frames (bf16w: on bf16-rounded weights; the
    probe tail and conv_post are bf16-exact already)."""
    key = (name, precision == "bf16w", b, n)
    if key not in _WAV64:
        _WAV64[key] = N.generator_forward(_gen_sd(name, precision), S.GEN_CONFIGS[name],
                                          np.array(S.gen_mel(name))[b:b + 1, :, :n])
    return _WAV64[key]


def _ragged_mel(name):
    mel = np.array(S.gen_mel(name))
    for b, n in enumerate(S.GEN_LENS):
        mel[b, :, n:] = -77.0
    return mel


# (FUSE_POST, RB_CONC): the fused conv_post launch needs the one-launch-per-ResBlock schedule,
# which forwards this small leave for concurrent ResBlocks + mrf_combine unless RB_CONC is 0
GEN_SCHEDULES = {"fused_post": (1, 0), "own_post": (0, 0), "concurrent": (1, -1)}


@pytest.mark.parametrize("schedule", list(GEN_SCHEDULES))
@pytest.mark.parametrize("name", ["v1", "v2star"])
def test_generator_probe_tail_ragged(pkg, dev, sched, evidence, name, schedule):
    """lengths (4, 3, 2, 1) frames: last-stage lengths 1024 .. 256, one to three windows of every
    launch of the last stage (test_seams_host.py), -77 in the mel's padding.  Each item within
    1e-4 of its own float64 wav, bitwise its solo run, zero past its length; the stage tensors
    of the full batch under the stage bars.  FUSE_POST 1 and 0 on the one-launch-per-ResBlock
    schedule, and the default schedule of a forward this small (concurrent ResBlocks)."""
    fuse_post, conc = GEN_SCHEDULES[schedule]
    sched("FUSE_POST", fuse_post)
    sched("RB_CONC", conc)
    cfg = S.GEN_CONFIGS[name]
    lens = list(S.GEN_LENS)
    mel = _ragged_mel(name)
    r64, r32 = S.gen_refs(name)
    worst_w, worst_s = {}, {}
    for precision in S.PRECISIONS:
        gen = S.make_generator(pkg, name, precision, dev)
        h = gen.hip_handle(dev)
        out, summary = _profiled(h, lambda: gen(_t(mel, dev), lengths=lens))
        fused = any(k.startswith("resblock_bf16x3<") for k in summary) and \
            not any(k.startswith("conv_post") for k in summary)
        assert fused == (name == "v1" and schedule == "fused_post" and precision != "fp32"), sorted(summary)
        if schedule != "concurrent":
            assert "mrf_combine" not in summary, sorted(summary)
        with torch.no_grad():
            for b, n in enumerate(lens):
                solo = gen(_t(mel[b:b + 1, :, :n], dev))
                m = solo.shape[-1]
                assert m == S.C.out_len(cfg, n)
                assert torch.equal(out[b:b + 1, :, :m], solo), (precision, b)
                assert not out[b, :, m:].any(), (precision, b)
                err = float(np.abs(solo.cpu().numpy() - _wav64(name, precision, b, n)).max())
                worst_w[precision] = max(worst_w.get(precision, 0.0), err)
                assert err < S.ATOL, (precision, b, err)
            if precision == "bf16w":
                continue
            wav, stages = gen.forward_with_stages(_t(S.gen_mel(name), dev))
        for s, t in stages.items():
            got = t.cpu().numpy().astype(np.float64)
            cond = float(np.abs(r32[s] - r64[s]).max())
            bar = S.stage_bar(precision, float(np.abs(r32[s]).max()), cond)
            err = float(np.abs(got - r32[s]).max())
            worst_s[precision] = max(worst_s.get(precision, (0.0, "")), (err / bar, f"{s} {err:.2e}"))
            assert err <= bar, (precision, s, err, bar, cond)
        assert float(np.abs(wav.cpu().numpy() - r64["wav"]).max()) < S.ATOL, precision
    evidence("max wav err " + ", ".join(f"{p} {e:.2e}" for p, e in worst_w.items()) +
             "; worst stage (of its bar) " + ", ".join(f"{p} {v} ({r:.2f})" for p, (r, v) in worst_s.items()))


@pytest.mark.parametrize("conc", [0, -1])
@pytest.mark.parametrize("precision", S.PRECISIONS)
@pytest.mark.parametrize("name", ["v1", "v2star"])
def test_generator_probe_tail_ignores_stale_buffers(pkg, dev, sched, evidence, name, precision, conc):
    """The same ragged batch with the wav and the workspace pre-filled with 1e30 and with zeros:
    bitwise the same wavs, each item within 1e-4 of its float64 wav and zero past its length.
    The end-of-sequence mask hides what the buffers hold, not only exact zeros.  RB_CONC 0: V1
    ends in the fused conv_post launch; -1: the concurrent schedule such a small forward gets."""
    sched("RB_CONC", conc)
    cfg = S.GEN_CONFIGS[name]
    lens = list(S.GEN_LENS)
    B, T = len(lens), S.GEN_T
    gen = S.make_generator(pkg, name, precision, dev)
    h = gen.hip_handle(dev)
    mel = _t(_ragged_mel(name), dev)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev)
    out_len, ws_bytes = h.out_len(T), h.workspace_bytes(B, T)
    stream = torch.cuda.current_stream(dev).cuda_stream
    outs = []
    for fill in (1e30, 0.0):
        ws = torch.full((ws_bytes // 4 + 1,), fill, dtype=torch.float32, device=dev)
        wav = torch.full((B, 1, out_len), fill, dtype=torch.float32, device=dev)
        h.forward_ex(mel.data_ptr(), B, T, wav.data_ptr(), out_len, ws.data_ptr(), ws_bytes, stream,
                     lengths_ptr=lens_t.data_ptr())
        torch.cuda.synchronize()
        outs.append(wav.cpu().numpy())
    assert np.array_equal(outs[0], outs[1]), "stale buffer contents changed the wav"
    worst = 0.0
    for b, n in enumerate(lens):
        m = S.C.out_len(cfg, n)
        worst = max(worst, float(np.abs(outs[0][b:b + 1, :, :m] - _wav64(name, precision, b, n)).max()))
        assert not outs[0][b, :, m:].any(), b
    evidence(f"max wav err {worst:.2e}")
    assert worst < S.ATOL


# ----------------------------------------------------------------------------------------
# 3. persistent grid
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", S.SPLIT_PRECISIONS)
def test_persistent_grid_walks_several_windows(pkg, dev, sched, evidence, precision):
    """The C = 64, k = 7 probe ResBlock on B x windows >= 2 x the CU count, so each block of the
    persistent grid walks several windows: against float64, and bitwise the RB_PERSIST 0 run."""
    case = S.BY_NAME["c64_k7"]
    (w,) = [w for w in S.windows(pkg, case.name) if w.tag == "whole"]
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    B = 8
    n_win = -(-2 * n_cu // B)
    L = (n_win - 1) * w.W + w.halo + 2
    assert B * -(-L // w.W) >= 2 * n_cu
    x, ref = S.probe_ref(case.name, L, B)
    outs = {}
    for persist in (2, 0):
        sched("RB_PERSIST", persist)
        mod = S.make_module(pkg, case.blk, precision, dev)
        y, summary = _profiled(mod._handle_for(dev), lambda: mod(_t(x, dev)))
        assert any("persist" in k for k in summary) == bool(persist), sorted(summary)
        outs[persist] = y
    assert torch.equal(outs[2], outs[0])
    got = outs[2].cpu().numpy().astype(np.float64)
    err = float(np.abs(got - ref).max())
    bar = S.RTOL[precision] * max(1.0, float(np.abs(ref).max()))
    evidence(f"B {B} x {-(-L // w.W)} windows on {n_cu} CUs: max err {err:.3g}")
    assert err <= bar, _first_wrong(got, ref, bar, [w], L)
