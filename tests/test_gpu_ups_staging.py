"""The output-frame upsampler's input staging and epilogue (csrc/ups_bf16x3.hip) against the
polyphase upsampler, bit for bit.

The staging gives every lane of every wave one (frame quad, 4-channel quarter) sub-task and
wave 0 the two halo frames; the epilogue loads its bias before the first store and, at rate 2,
stores a channel pair's column tiles back to back.  None of that may change a bit: per output
element the MFMA sequence, the staged value max(v sx, 0.1 v sx), its split and the final
fma(acc, sc, bias) are the polyphase kernel's (conv1d_bf16x3<..., UPS>).

Reference: the same forward with the upsamplers on the polyphase kernel.  The schedule value
that forced it everywhere (UPS_FRAMES=0) was removed in round 4 and is refused by the library
(tests/test_capi_host.py::test_removed_knob_value_is_refused), so the reference handle is
created under UPS_FRAMES=1, which keeps grids this small on the polyphase kernel, and every
test asserts from the launch profile that the reference ran no ups_bf16x3 launch and the run
under test (UPS_FRAMES=2) ran the expected ones.

The kernel runs a stage only when its input length is a multiple of 4 (csrc/forward.cpp
run_ups), so an item end at every position of a frame quad is a ragged item of a batch whose
width is a multiple of 4; hfg_forward_taps takes no lengths, so ragged batches are compared on
the wav and full batches on the ups taps and the wav.  All comparisons are torch.equal.
"""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu
PRECISIONS = ["f16x3", "bf16x3", "bf16w"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _cfg(c0, rates):
    from oracle import config as C
    return C.GenConfig(upsample_rates=list(rates), upsample_kernel_sizes=[2 * u for u in rates],
                       upsample_initial_channel=c0, resblock_kernel_sizes=[3, 5],
                       resblock_dilation_sizes=[[1, 3], [1]])


def _state(cfg, seed):
    from oracle import config as C
    return C.make_state_dict(cfg, seed=seed)


def _gen(pkg, cfg, sd, dev, precision, mode):
    """A module whose handle is created under UPS_FRAMES=mode; the knob is dropped again."""
    try:
        pkg.schedule_override("UPS_FRAMES", int(mode))
        gen = pkg.HiFiGANGenerator(**cfg.kwargs(), precision=precision).eval()
        gen.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        gen = gen.to(dev)
        gen.hip_handle(dev)
    finally:
        pkg.schedule_clear("UPS_FRAMES")
    return gen


def _frames_launches(summary):
    """{configuration: launches} of ups_bf16x3<WAVES_M, WAVES_N, WM, WN, np, fmt>."""
    out = {}
    for n, v in summary.items():
        m = re.fullmatch(r"ups_bf16x3<(\d+), (\d+), (\d+), (\d+), \d+, \d+>", n)
        if m:
            cfg = {(2, 2, 1, 4): 0, (1, 4, 1, 2): 1}[tuple(int(x) for x in m.groups())]
            out[cfg] = out.get(cfg, 0) + v["launches"]
    return out


def _plan_frames(gen, dev):
    """{upsampler module: (configuration, m-tiles)} of the handle's plan."""
    return {L["mod"]: tuple(L["frames"][:2]) for L in gen.hip_handle(dev).plan()["layers"]
            if re.fullmatch(r"ups\.\d", L["mod"])}


def _profiled(gen, dev, fn):
    h = gen.hip_handle(dev)
    h.profile_reset()
    h.set_profiling(True)
    with torch.no_grad():
        out = fn()
    torch.cuda.synchronize()
    h.set_profiling(False)
    return out, _frames_launches(h.profile_summary())


def _both(pkg, cfg, sd, dev, precision, fn, want):
    """fn(gen) under the polyphase reference and under the output-frame kernel; `want`:
    {configuration: launches} the run under test must show."""
    ref_gen = _gen(pkg, cfg, sd, dev, precision, 1)
    ref, n_ref = _profiled(ref_gen, dev, lambda: fn(ref_gen))
    assert n_ref == {}, f"reference ran the kernel under test: {n_ref}"
    new_gen = _gen(pkg, cfg, sd, dev, precision, 2)
    new, n_new = _profiled(new_gen, dev, lambda: fn(new_gen))
    assert n_new == want, (n_new, want)
    return ref, new, new_gen


def _mel(seed, B, T, dev):
    from oracle import prng
    return torch.as_tensor(prng.mel_input(seed, (B, 80, T))).to(dev)


def _equal_taps(ref, new):
    (rw, rt), (nw, nt) = ref, new
    assert torch.equal(rw, nw)
    for name in rt:
        if name.startswith("ups."):
            assert torch.equal(rt[name], nt[name]), name


# 128 -> 64 -> 32 channels at rates (8, 2): rows_f = 256 (configuration 0, 4 m-tiles) and 32
# (configuration 1, 1 m-tile), the smallest widths that put one stage on each tile
SEAM = (128, (8, 2))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("T,lens", [(8, [5, 6, 7, 8]), (260, [255, 256, 257, 260]),
                                    (260, [260, 250, 243])])
def test_staging_seams_ragged(pkg, dev, precision, T, lens):
    """Item ends at every position of a frame quad (5 .. 8), on both sides of the 256-frame
    tile edge (255, 256, 257, 260; the second stage sees 8 x these: 2048 is a tile edge too),
    and three items ending in different quads of one tile."""
    cfg = _cfg(*SEAM)
    sd = _state(cfg, 71)
    mel = _mel(71 + T, len(lens), T, dev)
    ref, new, gen = _both(pkg, cfg, sd, dev, precision, lambda g: g(mel, lengths=lens),
                          {0: 1, 1: 1})
    assert _plan_frames(gen, dev) == {"ups.0": (0, 4), "ups.1": (1, 1)}
    assert torch.equal(ref, new)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("T", [8, 260])
def test_staging_seams_taps(pkg, dev, precision, T):
    """Full batches of the same two-stage configuration: both upsampler outputs and the wav."""
    cfg = _cfg(*SEAM)
    sd = _state(cfg, 71)
    mel = _mel(72 + T, 2, T, dev)
    ref, new, _ = _both(pkg, cfg, sd, dev, precision, lambda g: g.forward_with_stages(mel),
                        {0: 1, 1: 1})
    _equal_taps(ref, new)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("c0,frames", [(16, (1, 1)), (32, (0, 1)), (48, (1, 3))])
def test_ring_parity_and_group_count(pkg, dev, precision, c0, frames):
    """C_in = 16, 32, 48: one, two and three 16-channel groups, i.e. the prologue alone, one
    swap of the two LDS slots, and a slot that is written a second time."""
    cfg = _cfg(c0, (8,))
    sd = _state(cfg, 73)
    full = _mel(73 + c0, 2, 12, dev)
    want = {frames[0]: 1}
    ref, new, gen = _both(pkg, cfg, sd, dev, precision, lambda g: g.forward_with_stages(full), want)
    assert _plan_frames(gen, dev) == {"ups.0": frames}
    _equal_taps(ref, new)
    ref, new, _ = _both(pkg, cfg, sd, dev, precision, lambda g: g(full, lengths=[12, 9]), want)
    assert torch.equal(ref, new)


def _forward_on(gen, dev, mel, lens, ws):
    """hfg_forward_ex on the caller's workspace `ws` (uint8)."""
    h = gen.hip_handle(dev)
    B, _, T = mel.shape
    out_len = h.out_len(T)
    wav = torch.empty((B, 1, out_len), dtype=torch.float32, device=dev)
    ln = torch.tensor(lens, dtype=torch.int32, device=dev)
    assert ws.numel() >= h.workspace_bytes(B, T)
    torch.cuda.current_stream(dev).synchronize()
    h.forward_ex(mel.contiguous().data_ptr(), B, T, wav.data_ptr(), out_len, ws.data_ptr(),
                 ws.numel(), torch.cuda.current_stream(dev).cuda_stream, lengths_ptr=ln.data_ptr())
    torch.cuda.synchronize()
    return wav


@pytest.mark.parametrize("precision", PRECISIONS)
def test_padding_rows_hold_no_data(pkg, dev, precision):
    """The frames in [T_b, L) of a ragged item are never read as data: on a workspace whose
    every byte is 0xFF (NaN bit patterns) the shorter item, which ends mid-quad, gives
    bitwise its solo run.  A sub-task that dropped the okt select would stage NaN."""
    cfg = _cfg(*SEAM)
    sd = _state(cfg, 74)
    gen = _gen(pkg, cfg, sd, dev, precision, 2)
    T, lens = 12, [12, 7]
    mel = _mel(75, 2, T, dev)
    h = gen.hip_handle(dev)
    ws = torch.full((h.workspace_bytes(2, T),), 0xFF, dtype=torch.uint8, device=dev)
    wav, n = _profiled(gen, dev, lambda: _forward_on(gen, dev, mel, lens, ws))
    assert n == {0: 1, 1: 1}, n
    hop = 16
    assert torch.isfinite(wav[1, :, :lens[1] * hop]).all()
    for b, nb in enumerate(lens):
        with torch.no_grad():
            solo = gen(mel[b:b + 1, :, :nb].contiguous())
        assert torch.equal(wav[b:b + 1, :, :nb * hop], solo), b


# one stage per rate class, on each tile the class can run on: (c0, u, (configuration, m-tiles))
RATE_CASES = [(32, 8, (0, 1)), (16, 8, (1, 1)),      # h = 4: 16-B stores per class
              (64, 4, (0, 1)), (32, 4, (1, 1)),      # h = 2: rows x classes = 4 samples
              (128, 2, (0, 1)), (64, 2, (1, 1))]     # h = 1: the DPP pair path


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("c0,u,frames", RATE_CASES)
def test_rate_classes(pkg, dev, precision, c0, u, frames):
    """u = 8, 4 and 2, one stage each.  The item of 9 frames has an odd length: at u = 2 its
    last frame has no partner and takes the 8-B fallback of the pair path.  (A batch of width
    9 would not run the kernel at all, so 9 is an item of a 12-frame batch.)"""
    cfg = _cfg(c0, (u,))
    sd = _state(cfg, 76)
    mel = _mel(76 + u, 2, 12, dev)
    want = {frames[0]: 1}
    ref, new, gen = _both(pkg, cfg, sd, dev, precision, lambda g: g(mel, lengths=[12, 9]), want)
    assert _plan_frames(gen, dev) == {"ups.0": frames}
    assert torch.equal(ref, new)
    ref, new, _ = _both(pkg, cfg, sd, dev, precision, lambda g: g.forward_with_stages(mel), want)
    _equal_taps(ref, new)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_run_to_run_after_dirty_lds(pkg, dev, precision):
    """The same ragged forward before and after an unrelated, louder forward that leaves other
    bytes in LDS: bitwise equal (staged rows and slab slots are written before they are read)."""
    from oracle import config as C
    cfg = _cfg(*SEAM)
    sd = _state(cfg, 77)
    gen = _gen(pkg, cfg, sd, dev, precision, 2)
    ocfg = C.PRESETS["v2star"]
    osd = {k: v * 4.0 for k, v in _state(ocfg, 78).items()}
    other = _gen(pkg, ocfg, osd, dev, precision, 2)
    omel = 30.0 * _mel(79, 3, 332, dev)
    mel, lens = _mel(80, 3, 260, dev), [260, 250, 243]
    outs = []
    with torch.no_grad():
        for _ in range(3):
            outs.append(gen(mel, lengths=lens).clone())
            other(omel)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
