"""Channel widths off the power-of-two grid on the GPU (tests/width_cases.py; the host side:
test_widths_host.py): partial 16-channel groups, row tails of the 32-row MFMA blocks and
part-full m-tiles, tile 3 as an LDS-ring layer conv, several m-tiles of the output-frame
upsampler, chunk tails of the fp32 kernel, 17-31-channel stages, conv_post / absmax /
mrf_combine at odd channel counts.

* every stage of every configuration against the fp32 oracle under the stage bars of
  test_gpu_stages.py (cond from the float64 oracle), the wav under the project's 1e-4, on the
  layers' own tiles and on the small tile, with the kernel instances that ran checked against
  the plan;
* the bitwise invariances the design claims, at these widths: small tile or not, output-frame
  or polyphase upsampler, one stream or two;
* ragged batches (both mel layouts), a NaN item beside finite ones, the standalone MRF /
  ResBlock entry at ten widths, conv_post in both kernels, and a seeded sweep over widths.
"""
import functools

import numpy as np
import pytest
import torch

import width_cases as W
from dynamic_range_cases import Block, _block_ref, make_module, region_check

pytestmark = pytest.mark.gpu
NAMES = list(W.CONFIGS)
SPLIT_PRECISIONS = ("f16x3", "bf16x3", "bf16w")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _profiled(h, fn):
    h.profile_reset()
    h.set_profiling(True)
    with torch.no_grad():
        out = fn()
    torch.cuda.synchronize()
    h.set_profiling(False)
    return out, h.profile_summary()


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def _check_instances(pkg, name, precision, small, summary):
    """The layer launches ran exactly the kernel instances the plan names for this SMALL_TILE:
    the layer's own tile (tile 3 where the plan says 3, not its AREG twin) or the small one."""
    plan = W.host_handle(pkg, name, precision).plan()
    split, fp32 = W.expected_instances(plan, W.gen_taps(W.CONFIGS[name]), small)
    assert W.bf16x3_instances(summary) == split, (sorted(summary), sorted(split))
    assert W.fp32_instances(summary) == fp32, (sorted(summary), sorted(fp32))
    assert "mrf_combine" in summary, sorted(summary)
    assert ("absmax" in summary) == (precision in ("f16x3", "bf16w")), sorted(summary)
    return split, fp32


# ----------------------------------------------------------------------------------------
# stage parity
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("small", [0, 1])
@pytest.mark.parametrize("precision", W.STAGE_PRECISIONS)
@pytest.mark.parametrize("name", NAMES)
def test_stage_parity(pkg, dev, sched, evidence, name, precision, small):
    sched("SMALL_TILE", small)
    gen = W.make_generator(pkg, name, precision, dev)
    h = gen.hip_handle(dev)
    (wav, stages), summary = _profiled(h, lambda: gen.forward_with_stages(_t(W.mel(name), dev)))
    split, fp32 = _check_instances(pkg, name, precision, small, summary)
    _, r32 = W.refs(name)
    bars = W.stage_bars(name, precision)
    worst = (0.0, None)
    for stage in W.stage_names(name):
        got = stages[stage].cpu().numpy()
        assert got.shape == r32[stage].shape, stage
        err = float(np.abs(got - r32[stage]).max())
        bar, cond, scale = bars[stage]
        print(f"{stage}: err {err:.3e} bar {bar:.3e} (max|ref| {scale:.3g}, fp32-vs-fp64 {cond:.2e})")
        worst = max(worst, (err / bar, f"{stage} err {err:.3e} bar {bar:.3e}"))
        assert err <= bar, (stage, err, bar, cond, scale)
    werr = float(np.abs(wav.cpu().numpy() - r32["wav"]).max())
    evidence(f"worst stage {worst[1]} ({worst[0]:.2f} of the bar); wav err {werr:.3e}; "
             f"split instances (kt, tile, ups) {sorted(split)}; fp32 (kt, tile, CK, ups) {sorted(fp32)}")
    assert werr < W.ATOL, werr
    with torch.no_grad():
        assert torch.equal(gen(_t(W.mel(name), dev)), wav)


@pytest.mark.parametrize("small", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_bf16w_wav_parity(pkg, dev, sched, evidence, name, small):
    """bf16w: the wav within 1e-4 of the oracle on bf16-rounded weights (the model the mode
    computes), as the config sweep does; its stage errors are reported, not asserted."""
    sched("SMALL_TILE", small)
    gen = W.make_generator(pkg, name, "bf16w", dev)
    h = gen.hip_handle(dev)
    (wav, stages), summary = _profiled(h, lambda: gen.forward_with_stages(_t(W.mel(name), dev)))
    _check_instances(pkg, name, "bf16w", small, summary)
    ref = W.refs_bf16w(name)
    rel = max((float(np.abs(stages[s].cpu().numpy() - ref[s]).max()) /
               max(1.0, float(np.abs(ref[s]).max())), s) for s in W.stage_names(name))
    werr = float(np.abs(wav.cpu().numpy() - ref["wav"]).max())
    evidence(f"wav err {werr:.3e}; worst stage {rel[1]} rel err {rel[0]:.3e}")
    assert werr < W.ATOL, werr


# ----------------------------------------------------------------------------------------
# bitwise invariances
# ----------------------------------------------------------------------------------------
LENS = [W.STAGE_T, 17, 1]


def _ragged_mel(name):
    mel = np.array(W.mel(name, 3, W.STAGE_T))
    for b, n in enumerate(LENS):
        mel[b, :, n:] = -77.0
    return mel


@pytest.mark.parametrize("precision", SPLIT_PRECISIONS)
@pytest.mark.parametrize("name", NAMES)
def test_small_tile_is_bitwise_invisible(pkg, dev, sched, name, precision):
    mel = _t(_ragged_mel(name), dev)
    outs, inst = {}, {}
    for small in (0, 1):
        sched("SMALL_TILE", small)
        gen = W.make_generator(pkg, name, precision, dev)
        h = gen.hip_handle(dev)
        outs[small], summary = _profiled(h, lambda: (gen.forward_with_stages(mel[:2]),
                                                     gen(mel, lengths=LENS)))
        inst[small] = W.bf16x3_instances(summary)
    assert inst[0] != inst[1] and any(t == 4 for _, t, _ in inst[1]) \
        and not any(t == 4 for _, t, _ in inst[0]), inst
    (wav0, st0), rag0 = outs[0]
    (wav1, st1), rag1 = outs[1]
    assert torch.equal(wav0, wav1) and torch.equal(rag0, rag1)
    for s in st0:
        assert torch.equal(st0[s], st1[s]), s


@pytest.mark.parametrize("precision", SPLIT_PRECISIONS)
@pytest.mark.parametrize("name,cfgs", [("W96", {0}), ("W160", {1}), ("W320", {0})])
def test_output_frame_upsampler_is_bitwise_the_polyphase_one(pkg, dev, sched, name, cfgs,
                                                              precision):
    """UPS_FRAMES 2 runs ups_bf16x3 wherever the plan packed it (W96: cfg 0 x 3 m-tiles, W160:
    cfg 1 x 5, W320: cfg 0 x 10 and x 5), UPS_FRAMES 1 only where its grid fills the chip (not
    at these sizes): the same bits, full and ragged."""
    mel = _t(_ragged_mel(name), dev)
    outs, frames = {}, {}
    for mode in (1, 2):
        sched("UPS_FRAMES", mode)
        gen = W.make_generator(pkg, name, precision, dev)
        h = gen.hip_handle(dev)
        outs[mode], summary = _profiled(h, lambda: (gen.forward_with_stages(mel[:2]),
                                                    gen(mel, lengths=LENS)))
        frames[mode] = W.ups_frames_launches(summary)
    plan = W.host_handle(pkg, name, precision).plan()
    packed = [tuple(L["frames"][:2]) for L in plan["layers"] if L["frames"][0] >= 0]
    assert {c for c, _ in packed} == cfgs and max(m for _, m in packed) >= 3, packed
    assert set(frames[2]) == cfgs and sum(frames[2].values()) > sum(frames[1].values()), frames
    # every packed upsampler ran on it, in the full and in the ragged forward
    assert sum(frames[2].values()) == 2 * len(packed), frames
    (wav1, st1), rag1 = outs[1]
    (wav2, st2), rag2 = outs[2]
    assert torch.equal(wav1, wav2) and torch.equal(rag1, rag2)
    for s in st1:
        assert torch.equal(st1[s], st2[s]), s


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("name", ["ODD100", "W160"])
def test_two_streams_are_bitwise_one(pkg, dev, name, precision):
    """A batch of 3 on one stream and as halves (2 + 1 items) on two.  The library splits a
    forward only from B x T = 4096 frames (plan.cpp split_batch), so this test alone runs long
    inputs, T = 1366, on the two configurations with the smallest rates; no oracle."""
    T = 1366
    cfg = W.CONFIGS[name]
    mel = _t(W.mel(name, 3, T), dev)
    lens = [T, 1001, 3]
    gen = W.make_generator(pkg, name, precision, dev)
    h = gen.hip_handle(dev)
    assert 3 * T >= 4096
    outs = []
    for n in (1, 2, 1):
        h.set_streams(n)
        with torch.no_grad():
            outs.append((gen(mel), gen(mel, lengths=lens)))
        torch.cuda.synchronize()
    h.set_streams(2)
    assert outs[0][0].shape[-1] == T * int(np.prod(cfg.upsample_rates))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    for a, b in zip(outs[0], outs[2]):
        assert torch.equal(a, b)


# ----------------------------------------------------------------------------------------
# ragged batches, both mel layouts
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["bct", "btc"])
@pytest.mark.parametrize("name", NAMES)
def test_ragged_items_equal_their_solo_runs(pkg, dev, evidence, name, layout):
    """lens [T, 17, 1], -77 in the padding: each item is bitwise its solo run, zero past its
    length and within 1e-4 of the oracle on its own frames (bf16w: on bf16-rounded weights)."""
    cfg = W.CONFIGS[name]
    mel = _ragged_mel(name)

    def arrange(m):
        m = torch.from_numpy(np.ascontiguousarray(m))
        return (m.transpose(1, 2).contiguous() if layout == "btc" else m).to(dev)

    worst = {}
    for precision in W.PRECISIONS:
        gen = W.make_generator(pkg, name, precision, dev)
        with torch.no_grad():
            out = gen(arrange(mel), lengths=LENS, mel_layout=layout)
            for b, n in enumerate(LENS):
                solo = gen(arrange(mel[b:b + 1, :, :n]), mel_layout=layout)
                m = solo.shape[-1]
                assert m == W.C.out_len(cfg, n)
                assert torch.equal(out[b:b + 1, :, :m], solo), (precision, b)
                assert not out[b, :, m:].any(), (precision, b)
                ref = W.wav_ref(name, 3, W.STAGE_T, precision == "bf16w", n, b)
                err = float(np.abs(solo.cpu().numpy() - ref).max())
                worst[precision] = max(worst.get(precision, 0.0), err)
                assert err < W.ATOL, (precision, b, err)
    evidence("max wav err " + ", ".join(f"{p} {e:.2e}" for p, e in worst.items()))


@pytest.mark.parametrize("precision", W.PRECISIONS)
@pytest.mark.parametrize("name", ["W320", "ODD100"])
def test_nan_item_leaves_its_neighbours_alone(pkg, dev, name, precision):
    """The last item's mel is all NaN (f16x3: its scale slots hold NaN maxima; every kernel's
    masked tail loads read NaN): every other item is bitwise its solo run."""
    mel = np.array(W.mel(name, 3, W.STAGE_T))
    mel[2] = np.nan
    gen = W.make_generator(pkg, name, precision, dev)
    with torch.no_grad():
        out = gen(_t(mel, dev))
        for b in (0, 1):
            solo = gen(_t(mel[b:b + 1], dev))
            assert torch.isfinite(solo).all()
            assert torch.equal(out[b:b + 1], solo), b
    assert torch.isnan(out[2]).any()


# ----------------------------------------------------------------------------------------
# standalone MRF / ResBlock entry
# ----------------------------------------------------------------------------------------
def _mrf_block(width, j):
    return Block(f"w{width}", width, tuple(W.RES_KERNELS), W.MRF_DILATIONS, j=j, seed=300 + width)


@functools.lru_cache(maxsize=None)
def _mrf_case(width, L):
    """(x f32[2, C, L], {j: BlockRef}) with j = -1 the whole MRF; computed once and shared."""
    x = W.prng.normal(300 + width, f"x{L}", (2, width, L), 0.5)
    x.setflags(write=False)
    return x, {j: _block_ref(_mrf_block(width, j), x) for j in (-1, 0, 1, 2)}


@pytest.mark.parametrize("small", [0, 1])
@pytest.mark.parametrize("L", W.MRF_LENGTHS)
@pytest.mark.parametrize("width", W.MRF_WIDTHS)
def test_standalone_mrf_and_resblocks(pkg, dev, sched, evidence, width, L, small):
    """hfg_mrf_create at each width: the MRF and each of its ResBlocks (k = 3, 7, 11, dilations
    [1, 3]) on x [2, C, L] against the float64 restatement under the stage bar.  (The entry
    takes no lengths: the two items differ, neither is padded.)"""
    sched("SMALL_TILE", small)
    x, refs = _mrf_case(width, L)
    worst = {}
    for precision in W.STAGE_PRECISIONS:
        mrf = make_module(pkg, _mrf_block(width, -1), precision, dev)
        for j, ref in refs.items():
            if j < 0:
                # the whole MRF ran the instances its plan names: every width from 32 on the
                # split-precision kernel (the small tile where forced and packed), 20 - 25 the
                # fp32 one
                h = mrf._handle_for(dev)
                y, summary = _profiled(h, lambda: mrf(_t(x, dev)))
                want = W.expected_instances(h.plan(), W.mrf_taps(), small)
                assert (W.bf16x3_instances(summary), W.fp32_instances(summary)) == want, \
                    (sorted(summary), want)
                assert bool(want[0]) == (precision != "fp32" and width >= 32)
            else:
                with torch.no_grad():
                    y = mrf.resblocks[j](_t(x, dev))
            err, bar, cond, scale = region_check(y.cpu().numpy(), ref.ref64, ref.ref32, None,
                                                 W.STAGE_RTOL[precision])
            worst[precision] = max(worst.get(precision, (0.0, 0.0)), (err / bar, err))
            assert err <= bar, (precision, j, err, bar, cond, scale)
    evidence("worst err (of its bar) " + ", ".join(f"{p} {e:.2e} ({r:.2f})"
                                                   for p, (r, e) in worst.items()))


# ----------------------------------------------------------------------------------------
# conv_post
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("name,T,kernel", [("W200R", 33, "conv_post_tanh"),
                                           ("W400", 40, "conv_post4_tanh"),
                                           ("ODD100", 40, "conv_post4_tanh")])
def test_conv_post_at_odd_channel_counts(pkg, dev, name, T, kernel, precision):
    """C = 50 in the LDS-staged kernel (32 + 18 channels; L = 495) and in the quad kernel,
    C = 12 in the kernel its L selects; full and ragged against the oracle."""
    cfg = W.CONFIGS[name]
    assert (W.C.out_len(cfg, T) % 4 == 0) == (kernel == "conv_post4_tanh")
    lens = [T, 17, 1]
    mel = np.array(W.mel(name, 3, T))
    gen = W.make_generator(pkg, name, precision, dev)
    h = gen.hip_handle(dev)
    (full, rag), summary = _profiled(h, lambda: (gen(_t(mel, dev)),
                                                 gen(_t(mel, dev), lengths=lens)))
    other = ({"conv_post_tanh", "conv_post4_tanh"} - {kernel}).pop()
    assert kernel in summary and other not in summary, sorted(summary)
    assert summary[kernel]["launches"] == 2
    err = float(np.abs(full.cpu().numpy() - W.wav_ref(name, 3, T)).max())
    assert err < W.ATOL, err
    for b, n in enumerate(lens):
        m = W.C.out_len(cfg, n)
        ref = W.wav_ref(name, 3, T, False, n, b)
        assert float(np.abs(rag[b:b + 1, :, :m].cpu().numpy() - ref).max()) < W.ATOL, b
        assert not rag[b, :, m:].any(), b


# ----------------------------------------------------------------------------------------
# width sweep
# ----------------------------------------------------------------------------------------
def _draw(seed):
    """test_gpu_config_sweep's draw with the channel width and the mel bins off the grid."""
    r = np.random.default_rng(2000 + seed)
    n_up = int(r.integers(1, 5))
    c0 = int(r.choice(W.SWEEP_C0))
    n_mels = int(r.choice(W.SWEEP_MELS))
    rates, kernels = [], []
    for _ in range(n_up):
        u = int(r.choice([2, 3, 4, 5, 8]))
        k = int(r.choice([u, 2 * u, 2 * u + 1, 2 * u - 1 if u > 1 else u]))
        rates.append(u)
        kernels.append(max(k, 1))
    n_res = int(r.integers(1, 4))
    ks = [int(r.choice([3, 5, 7, 11])) for _ in range(n_res)]
    dils = [[int(d) for d in r.choice([1, 2, 3, 5], size=int(r.integers(1, 4)))] for _ in range(n_res)]
    cfg = W.C.GenConfig(n_mels=n_mels, upsample_rates=rates, upsample_kernel_sizes=kernels,
                        upsample_initial_channel=c0, resblock_kernel_sizes=ks,
                        resblock_dilation_sizes=dils)
    B = int(r.integers(1, 4))
    T = int(r.integers(3, 33))
    lens = [T] + [int(r.integers(1, T + 1)) for _ in range(B - 1)]
    return cfg, lens


@pytest.mark.parametrize("seed", range(W.SWEEP_SEEDS))
def test_random_width_config(pkg, dev, seed):
    """The contract of test_gpu_config_sweep.test_random_config at widths off the grid: a
    configuration is either accepted and within 1e-4 of the oracle with every ragged item
    bitwise its solo run, or refused at creation with a message."""
    from oracle import hifigan_torch as H
    cfg, lens = _draw(seed)
    sd = W.C.make_state_dict(cfg, seed=seed)
    rounded = W.bf16_rounded(sd)
    T = max(lens)
    mel = torch.randn(len(lens), cfg.n_mels, T, generator=torch.Generator().manual_seed(seed))
    refs_by = {}
    for key, w in (("fp32", sd), ("bf16", rounded)):
        refs_by[key] = [H.generator_forward(H.to_torch_state(w), cfg, mel[b:b + 1, :, :n])
                        for b, n in enumerate(lens)]
    print(f"\nseed {seed}: {cfg} lens {lens}")
    for precision in ("fp32", "f16x3", "bf16x3", "bf16w"):
        refs = refs_by["bf16" if precision == "bf16w" else "fp32"]
        gen = pkg.HiFiGANGenerator(**cfg.kwargs(), precision=precision).eval()
        gen.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        gen = gen.to(dev)
        try:
            gen.hip_handle(dev)
        except Exception as e:  # refused configurations: at creation, with a reason
            msg = str(e)
            print(f"  {precision}: refused at creation: {msg}")
            assert msg, "refusal without a message"
            continue
        with torch.no_grad():
            out = gen(mel.to(dev), lengths=lens)
            for b, n in enumerate(lens):
                solo = gen(mel[b:b + 1, :, :n].contiguous().to(dev))
                m = solo.shape[-1]
                assert m == refs[b].shape[-1]
                assert torch.equal(out[b:b + 1, :, :m], solo), (precision, b)
                err = (solo.cpu() - refs[b]).abs().max().item()
                assert err < W.ATOL, (precision, b, err)
        torch.cuda.synchronize()
        print(f"  {precision}: ok")
