"""The Generator's argument edges on the GPU (cases, inputs and references:
tests/argument_cases.py; their CPU half and the mutants that show each check can fail:
tests/test_arguments_host.py).

1. Lengths outside [1, T]: wild device lengths (10^9, negative, 0, T + 1, INT32_MIN) with NaN in
   every padded frame and in every empty item.  The wav is bitwise the forward on the clamped
   lengths, every item bitwise its solo run and zero past its own output, every empty item a
   zero row, everything finite, and the float64 reference within 1e-4 — under every schedule
   that places an empty item differently, on a large ragged batch whose empty items sit first,
   last or alone in a stream's half, and on a batch of nothing but empty items.
2. Guards: ``mel`` in an arena of NaN, ``wav`` / tap buffers / ``y`` in arenas of -7.5, the
   lengths in an arena of 10^9, the workspace between bands: no band changes and the output is
   bitwise the module's forward.  A correct kernel never touches a band or uses a value from
   one: nothing here provokes an out-of-bounds access.
3. The batch axis: B = 65536 is refused with HFG_EINVAL before anything runs, B = 65535 runs on
   a thin-MRF and on a whole-ResBlock configuration, one stream (grids of 65535) and two.
4. A batch whose activation buffers pass 4 GiB (V1, 5 x 32768 frames: item 2 starts 2^31 bytes
   into a buffer, item 4 exactly 2^32): every item bitwise its solo run.
"""
import ctypes
import time

import numpy as np
import pytest
import torch

import argument_cases as A
from oracle import config as C, hifigan_torch as H

pytestmark = pytest.mark.gpu
ATOL = A.ATOL


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def run(gen, mel, **kw):
    with torch.no_grad():
        out = gen(mel, **kw)
    torch.cuda.synchronize()
    return out


def _assert_items_are_solo(gen, mel, wav, lens, what):
    """Item b of wav bitwise the solo run on mel[b, :, :lens[b]], zero past it; an empty item a
    zero row; the whole wav finite."""
    assert bool(torch.isfinite(wav).all()), what
    for b, n in enumerate(lens):
        if n == 0:
            assert not bool(wav[b].any()), (what, b, "empty item is not a zero row")
            continue
        solo = run(gen, mel[b:b + 1, :, :n].contiguous())
        m = solo.shape[-1]
        assert m == gen.output_length(n)
        assert torch.equal(wav[b:b + 1, :, :m], solo), (what, b, n)
        assert not bool(wav[b, :, m:].any()), (what, b, n, "nonzero past the item's output")


# ---- 1. wild and empty lengths ------------------------------------------------------------
def _wild_case(pkg, dev, evidence, name, precision, knobs):
    T = A.WILD_T
    lens = A.clamped(A.WILD, T)
    gen = A.make_generator(pkg, name, precision, dev, knobs)
    mel = torch.from_numpy(np.array(A.wild_mel(name))).to(dev)
    mel_btc = mel.transpose(1, 2).contiguous()
    wild = torch.tensor(A.WILD, dtype=torch.int32, device=dev)
    wav = run(gen, mel, lengths=wild)
    assert wav.shape == (len(lens), 1, C.out_len(A.CONFIGS[name], T))
    assert torch.equal(wav, run(gen, mel, lengths=lens))
    wav_btc = run(gen, mel_btc, lengths=wild, mel_layout="btc")
    assert torch.equal(wav_btc, run(gen, mel_btc, lengths=lens, mel_layout="btc"))
    _assert_items_are_solo(gen, mel, wav, lens, "bct")
    _assert_items_are_solo(gen, mel, wav_btc, lens, "btc")
    if precision in A.REF_PRECISIONS:
        err = 0.0
        for b in A.WILD_REF_ITEMS:
            ref = A.wild_ref(name, b)
            got = wav[b, 0, :ref.shape[0]].cpu().numpy().astype(np.float64)
            err = max(err, float(np.abs(got - ref).max()))
        evidence(f"wild lengths {name} [{precision}] {knobs or 'default'}: "
                 f"max|err| vs float64 {err:.2e}")
        assert err < ATOL


@pytest.mark.parametrize("precision", A.PRECISIONS)
@pytest.mark.parametrize("name", A.WILD_CONFIGS)
def test_wild_lengths(pkg, dev, evidence, name, precision):
    _wild_case(pkg, dev, evidence, name, precision, {})


SCHEDULES = [{"RB_CONC": 0}, {"RB_CONC": 1}, {"SMALL_TILE": 0}, {"SMALL_TILE": 1},
             {"FUSED_RB": 0}, {"FUSE_POST": 0}]


@pytest.mark.parametrize("knobs", SCHEDULES, ids=lambda k: "-".join(f"{a}={b}" for a, b in k.items()))
@pytest.mark.parametrize("precision", A.PRECISIONS)
@pytest.mark.parametrize("name", A.WILD_CONFIGS)
def test_wild_lengths_under_schedules(pkg, dev, evidence, name, precision, knobs):
    _wild_case(pkg, dev, evidence, name, precision, knobs)


RAGGED_T = 1100


@pytest.fixture(scope="module")
def ragged_mel():
    return torch.randn(4, 80, RAGGED_T, generator=torch.Generator().manual_seed(A.SEED + 4))


@pytest.mark.parametrize("precision", ["f16x3", "bf16x3"])
@pytest.mark.parametrize("lens", [[1100, 0, 1100, 0], [0, 0, 1100, 513]], ids=["x0x0", "00xy"])
def test_large_ragged_batch_with_empty_items(pkg, dev, evidence, ragged_mel, lens, precision):
    """V1 4 x 1100 with empty items first, last, or alone in a stream's half (two streams cut
    the batch into items 0-1 and 2-3), with and without the persistent ResBlock grid, which
    then sees items without a single window."""
    T = RAGGED_T
    mel = torch.from_numpy(A.nan_padded(ragged_mel.numpy(), lens)).to(dev)
    outs = {}
    for persist in (0, 2):
        gen = A.make_generator(pkg, "v1", precision, dev, {"RB_PERSIST": persist})
        h = gen.hip_handle(dev)
        for n in (1, 2):
            h.set_streams(n)
            assert len(h.workspace_layout(4, T)["parts"]) == n
            h.profile_reset()
            h.set_profiling(True)
            outs[persist, n] = run(gen, mel, lengths=lens)
            h.set_profiling(False)
            assert any("persist" in k for k in h.profile_summary()) == bool(persist), (persist, n)
        h.set_streams(1)
    _assert_items_are_solo(gen, mel, outs[0, 1], lens, "RB_PERSIST=0, 1 stream")
    for key, wav in outs.items():
        assert torch.equal(wav, outs[0, 1]), key
    # one 40-frame window of item 2 against the oracle
    a, e, m = 200, 240, 15
    ref = H.generator_forward(A.torch_state("v1"), C.V1,
                              ragged_mel[2:3, :, a - m:e + m])
    got = outs[2, 2][2:3, :, a * 256:e * 256].cpu()
    err = (got - ref[:, :, m * 256:(m + e - a) * 256]).abs().max().item()
    evidence(f"large ragged {lens} [{precision}]: item 2 window max|err| vs oracle {err:.2e}")
    assert err < ATOL


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", A.WILD_CONFIGS)
def test_all_empty_batch(pkg, dev, name, precision):
    """lengths = [0, 0, 0] on an all-NaN mel: a zero wav (a refused or failed forward raises),
    and the handle's next forward is bitwise a fresh handle's."""
    T = A.WILD_T
    cfg = A.CONFIGS[name]
    gen = A.make_generator(pkg, name, precision, dev)
    nothing = torch.full((3, cfg.n_mels, T), float("nan"), device=dev)
    for lens in ([0, 0, 0], torch.tensor([0, -1, -2 ** 31], dtype=torch.int32, device=dev)):
        wav = run(gen, nothing, lengths=lens)
        assert wav.shape == (3, 1, C.out_len(cfg, T))
        assert bool(torch.isfinite(wav).all()) and not bool(wav.any())
    mel = torch.from_numpy(np.nan_to_num(np.array(A.wild_mel(name)[:3]), nan=0.5)).to(dev)
    after = run(gen, mel, lengths=[T, T, T])
    fresh = run(A.make_generator(pkg, name, precision, dev), mel, lengths=[T, T, T])
    assert torch.equal(after, fresh)
    assert bool(after.any())


@pytest.mark.parametrize("name", ["v1", "nonexact"])
def test_vocode_acoustic_with_an_empty_item(pkg, dev, name):
    import importlib
    glue = importlib.import_module("tts_sambert_hifigan_amd.glue")
    T = A.WILD_T
    gen = A.make_generator(pkg, name, "f16x3", dev)
    lens = [T, 0, 5]
    mel = torch.from_numpy(A.nan_padded(A.wild_mel(name)[[0, 1, 3]], lens)).to(dev)
    with torch.no_grad():
        wavs = glue.vocode_acoustic(gen, mel.transpose(1, 2).contiguous(), lens)
    assert wavs[1].shape == (0,)
    for b in (0, 2):
        solo = run(gen, mel[b:b + 1, :, :lens[b]].contiguous())
        assert torch.equal(wavs[b], solo[0, 0]), b


# ---- 2. guarded arguments -------------------------------------------------------------------
GUARD_CASES = [
    # name, B, T, lengths, layout
    ("nonexact", 3, 1, None, "bct"), ("nonexact", 3, 33, None, "bct"),
    ("nonexact", 3, 33, [33, 20, 1], "bct"),
    ("tail", 3, 1, None, "bct"), ("tail", 3, 33, None, "bct"), ("tail", 3, 33, [33, 20, 1], "bct"),
    ("v1", 2, 40, None, "bct"),
    ("v2star", 3, 64, None, "bct"), ("v2star", 3, 64, None, "btc"),
]


def _guard_mel(name, B, T):
    from oracle import prng
    return prng.mel_input(A.SEED + 5 + T, (B, A.CONFIGS[name].n_mels, T))


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("name,B,T,lens,layout", GUARD_CASES,
                         ids=[f"{c[0]}-{c[1]}x{c[2]}{'-ragged' if c[3] else ''}-{c[4]}"
                              for c in GUARD_CASES])
def test_forward_ex_between_guards(pkg, dev, name, B, T, lens, layout, precision):
    gen = A.make_generator(pkg, name, precision, dev)
    m = _guard_mel(name, B, T)
    if lens:
        m = A.nan_padded(m, lens)
    src = torch.from_numpy(m).to(dev)
    if layout == "btc":
        src = src.transpose(1, 2).contiguous()
    want = run(gen, src, lengths=lens, mel_layout=layout)
    h = gen.hip_handle(dev)
    mel = A.Arena(src.shape, float("nan"), dev).put(src)
    wav = A.Arena(want.shape, -7.5, dev)
    lengths = A.Arena((B,), 10 ** 9, dev, torch.int32).put(torch.tensor(lens, dtype=torch.int32)) \
        if lens else None
    ws = A.Banded(h.workspace_bytes(B, T), dev)
    torch.cuda.synchronize()
    h.forward_ex(mel.t.data_ptr(), B, T, wav.t.data_ptr(), h.out_len(T), ws.ptr, ws.nbytes,
                 _stream(dev), mel_layout=layout,
                 lengths_ptr=lengths.t.data_ptr() if lengths else 0)
    ws.assert_bands_untouched()
    wav.assert_bands_untouched("wav")
    mel.assert_bands_untouched("mel")
    if lengths:
        lengths.assert_bands_untouched("lengths")
        assert lengths.t.tolist() == lens
    assert torch.equal(mel.t.view(torch.int32), src.view(torch.int32))  # the input is never modified
    assert bool(torch.isfinite(wav.t).all())
    assert torch.equal(wav.t, want)


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", ["nonexact", "tail"])
def test_forward_taps_between_guards(pkg, dev, name, precision):
    B, T = 3, 33
    gen = A.make_generator(pkg, name, precision, dev)
    src = torch.from_numpy(_guard_mel(name, B, T)).to(dev)
    with torch.no_grad():
        want, stages = gen.forward_with_stages(src)
    torch.cuda.synchronize()
    h = gen.hip_handle(dev)
    mel = A.Arena(src.shape, float("nan"), dev).put(src)
    wav = A.Arena(want.shape, -7.5, dev)
    taps = {k: A.Arena(v.shape, -7.5, dev) for k, v in stages.items()}
    ws = A.Banded(h.workspace_bytes(B, T), dev)
    torch.cuda.synchronize()
    h.forward_taps(mel.t.data_ptr(), B, T, wav.t.data_ptr(), h.out_len(T), ws.ptr, ws.nbytes,
                   [a.t.data_ptr() for a in taps.values()], _stream(dev))
    ws.assert_bands_untouched()
    wav.assert_bands_untouched("wav")
    assert bool(torch.isfinite(wav.t).all()) and torch.equal(wav.t, want)
    for k, a in taps.items():
        a.assert_bands_untouched(k)
        assert torch.equal(a.t, stages[k]), k


@pytest.mark.parametrize("fused_rb", [1, 0], ids=["default", "FUSED_RB=0"])
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("ch,L", [(64, 259), (32, 513)])
@pytest.mark.parametrize("block", ["mrf", "resblock"])
def test_mrf_entries_between_guards(pkg, dev, block, ch, L, precision, fused_rb):
    """hfg_mrf_forward (the reference's MRF of k = 3, 7, 11) and hfg_resblock_forward (one
    k = 7 ResBlock) at L % 4 == 3 and 1."""
    B = 2
    knobs = {} if fused_rb else {"FUSED_RB": 0}
    torch.manual_seed(A.SEED + ch)
    try:
        for k, v in knobs.items():
            pkg.schedule_override(k, v)
        mod = (pkg.MRF(ch, precision=precision) if block == "mrf" else
               pkg.ResBlock(ch, 7, (1, 3, 5), precision=precision)).eval().to(dev)
        src = (torch.randn(B, ch, L) * 0.5).to(dev)
        with torch.no_grad():
            want = mod(src)
    finally:
        for k in knobs:
            pkg.schedule_clear(k)
    h = mod._handle_for(dev)
    x = A.Arena(src.shape, float("nan"), dev).put(src)
    y = A.Arena(src.shape, -7.5, dev)
    ws = A.Banded(h.mrf_workspace_bytes(B, L), dev)
    torch.cuda.synchronize()
    h.mrf_forward(x.t.data_ptr(), B, L, y.t.data_ptr(), ws.ptr, ws.nbytes, _stream(dev),
                  resblock=-1 if block == "mrf" else 0)
    ws.assert_bands_untouched()
    y.assert_bands_untouched("y")
    x.assert_bands_untouched("x")
    assert torch.equal(x.t, src)
    assert bool(torch.isfinite(y.t).all())
    assert torch.equal(y.t, want)


# ---- 3. the batch axis ----------------------------------------------------------------------
def test_batch_over_the_limit_is_refused(pkg, dev):
    """B = 65536 is refused with EINVAL by every entry that takes a B, called with 64-float
    dummy buffers: none of them may touch one."""
    lib = pkg.load_library()
    B = A.MAX_BATCH + 1
    dummy = torch.full((64,), -7.5, device=dev)
    p = ctypes.c_void_p(dummy.data_ptr())
    gen = A.make_generator(pkg, "tiny128", "f16x3", dev)
    h = gen.hip_handle(dev)
    L = lib.hfg_out_len(h.ptr, 1)
    opts = pkg._lib.HfgForwardOpts(0, p)
    taps = (ctypes.c_void_p * 5)(*[dummy.data_ptr()] * 5)
    mrf = pkg.MRF(32, precision="f16x3").eval().to(dev)
    hm = mrf._handle_for(dev)
    calls = {
        "hfg_forward_ex": lambda: lib.hfg_forward_ex(h.ptr, p, B, 1, ctypes.byref(opts), p, L, p,
                                                     1 << 40, None),
        "hfg_forward_ws": lambda: lib.hfg_forward_ws(h.ptr, p, B, 1, p, L, p, 1 << 40, None),
        "hfg_forward": lambda: lib.hfg_forward(h.ptr, p, B, 1, p, L, None),
        "hfg_forward_taps": lambda: lib.hfg_forward_taps(h.ptr, p, B, 1, p, L, p, 1 << 40, taps, 5,
                                                         None),
        "hfg_reserve": lambda: lib.hfg_reserve(h.ptr, B, 1),
        "hfg_mrf_forward": lambda: lib.hfg_mrf_forward(hm.ptr, p, B, 4, ctypes.c_void_p(
            dummy.data_ptr() + 64), p, 1 << 40, None),
        "hfg_resblock_forward": lambda: lib.hfg_resblock_forward(hm.ptr, 0, p, B, 4, ctypes.c_void_p(
            dummy.data_ptr() + 64), p, 1 << 40, None),
    }
    for name, call in calls.items():
        assert call() == -22, name
        assert b"B must be in [1, 65535]" in lib.hfg_last_error(), name
    assert h.workspace_bytes(B, 1) == 0 and hm.mrf_workspace_bytes(B, 4) == 0
    torch.cuda.synchronize()
    assert bool((dummy == -7.5).all())
    with pytest.raises(RuntimeError, match=r"B must be in \[1, 65535\]"):
        gen(torch.empty(B, 80, 1, device=dev))
    with pytest.raises(RuntimeError, match=r"B must be in \[1, 65535\]"):
        mrf(torch.empty(B, 32, 4, device=dev))


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("name", ["tiny32", "tiny128"])
def test_batch_at_the_limit_runs(pkg, dev, evidence, name, precision):
    """B = 65535, T = 1: the batch is the whole of gridDim.y / gridDim.z on one stream, halves
    of 32768 and 32767 on two."""
    B = A.MAX_BATCH
    gen = A.make_generator(pkg, name, precision, dev)
    h = gen.hip_handle(dev)
    thin = [bool(s["thin"]) for s in h.plan()["stages"]]
    assert thin == ([True, True] if name == "tiny32" else [False, False])
    mel = torch.from_numpy(np.array(A.limit_mel(name))).to(dev)
    outs = {}
    for n, parts in ((1, [B]), (2, [32768, 32767])):
        h.set_streams(n)
        assert [p["B"] for p in h.workspace_layout(B, 1)["parts"]] == parts
        outs[n] = run(gen, mel)
    wav = outs[1]
    assert wav.shape == (B, 1, 4)
    assert bool(torch.isfinite(wav).all())
    assert torch.equal(outs[1], outs[2])
    refs = A.limit_ref(name)
    err = 0.0
    for b in A.LIMIT_ITEMS:
        assert torch.equal(wav[b:b + 1], run(gen, mel[b:b + 1].contiguous())), b
        err = max(err, float(np.abs(wav[b, 0].cpu().numpy().astype(np.float64) - refs[b]).max()))
    evidence(f"B = 65535 {name} [{precision}]: max|err| vs float64 over items "
             f"{list(A.LIMIT_ITEMS)} {err:.2e}")
    assert err < ATOL
    for i, a in enumerate(A.LIMIT_ITEMS):
        for b in A.LIMIT_ITEMS[i + 1:]:
            assert not torch.equal(wav[a], wav[b]), (a, b)
    # ragged: ten empty items planted among 65525 full ones
    zeros = A.planted_zeros(B)
    assert zeros[0] == 0 and zeros[-1] == B - 1
    lens = torch.ones(B, dtype=torch.int32)
    lens[zeros] = 0
    keep = lens.bool().to(dev)
    for n in (1, 2):
        h.set_streams(n)
        ragged = run(gen, mel, lengths=lens.to(dev))
        assert not bool(ragged[~keep].any()), n
        assert torch.equal(ragged[keep], wav[keep]), n
    h.set_streams(1)


# ---- 4. a batch past 4 GiB per buffer -------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_batch_past_4gib_per_buffer(pkg, dev, evidence, precision):
    """V1, 5 x 32768 frames: stages 1-3 hold 2^30 bytes per item, so item 2 starts 2^31 bytes
    into each activation buffer and item 4 exactly 2^32, where a base computed in 32 bits lands
    on item 0.  One stream: all five items in one part; two: parts of 3 and 2 items, the second
    part's buffers starting past 12 GiB."""
    t0 = time.perf_counter()
    B, T = A.HUGE_B, A.HUGE_T
    gen = A.make_generator(pkg, "v1", precision, dev)
    h = gen.hip_handle(dev)
    need = h.workspace_bytes(B, T) + 4 * B * 80 * T + 4 * B * h.out_len(T)
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info(dev)[0]
    if free < need:
        pytest.skip(f"{free >> 30} GiB free, the batch needs {need >> 30} GiB")
    mel = torch.randn(B, 80, T, generator=torch.Generator().manual_seed(A.SEED + 6))
    mel_d = mel.to(dev)
    outs = {}
    for n, parts in ((1, [5]), (2, [3, 2])):
        h.set_streams(n)
        lay = h.workspace_layout(B, T)
        assert [p["B"] for p in lay["parts"]] == parts
        if n == 2:
            assert all(r["off"] >= 12 * 2 ** 30 for r in lay["parts"][1]["regions"])
        outs[n] = run(gen, mel_d)
    h.set_streams(1)
    assert outs[1].shape == (B, 1, T * 256)
    for b in range(B):
        solo = run(gen, mel_d[b:b + 1].contiguous())
        for n in (1, 2):
            assert torch.equal(outs[n][b:b + 1], solo), (b, n)
        del solo
    assert not torch.equal(outs[1][4], outs[1][0])
    W, M = 32, 16
    tsd = A.torch_state("v1")
    err = 0.0
    for b in (2, 4):
        for start in (0, T // 2 + 5, T - W):
            lo, hi = max(0, start - M), min(T, start + W + M)
            ref = H.generator_forward(tsd, C.V1, mel[b:b + 1, :, lo:hi])
            ref = ref[0, 0, (start - lo) * 256:(start - lo + W) * 256]
            got = outs[2][b, 0, start * 256:(start + W) * 256].cpu()
            err = max(err, (got - ref).abs().max().item())
    del outs, mel_d
    torch.cuda.empty_cache()
    evidence(f"5 x 32768 V1 [{precision}]: items 2 and 4 windows max|err| vs oracle {err:.2e}; "
             f"test took {time.perf_counter() - t0:.1f} s")
    assert err < ATOL
