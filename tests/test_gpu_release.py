"""The public HiFi-GAN release's Generator on the GPU: ResBlock2 (release V3) through the
whole-ResBlock2 kernel (resblock2_bf16x3) and the layer path, and the release's final
leaky_relu slope 0.01 through all three conv_post kernels.  The oracle is the CPU
restatement of the release's forward, tests/release_oracle.py (asserted bitwise equal to
the reference oracle for the reference's architecture by test_release_host.py); the bar is
the project's 1e-4 on the wav."""
import importlib

import numpy as np
import pytest
import torch

from release_oracle import block_forward, release_forward, scaled

pytestmark = pytest.mark.gpu
ATOL = 1e-4
B, T, LENS = 3, 100, [100, 37, 2]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def S(pkg):
    import __graft_entry__ as ge
    return importlib.import_module(ge.PKG_NAME + ".synth")


def _bf16_weights(sd):
    return {k: (torch.from_numpy(v).to(torch.bfloat16).float().numpy() if k.endswith(".weight")
                else v) for k, v in sd.items()}


@pytest.fixture(scope="module")
def v3(S):
    """RELEASE_V3 weights (x1, x2), one mel, and each item's solo oracle wav on the fp32 and
    on the bf16-rounded weights: computed once, shared by the tests below, never modified."""
    cfg = S.RELEASE_V3
    base = S.random_state_dict(cfg, seed=17)
    mel = torch.randn(B, 80, T, generator=torch.Generator().manual_seed(17))
    case = {"cfg": cfg, "mel": mel, "sd": {}, "ref": {}}
    for scale in (1, 2):
        sd = scaled(base, float(scale))
        case["sd"][scale] = sd
        for name, w in (("fp32", sd), ("bf16", _bf16_weights(sd))):
            if name == "bf16" and scale != 1:
                continue
            case["ref"][scale, name] = [release_forward(w, cfg, mel[b:b + 1, :, :n])
                                        for b, n in enumerate(LENS)]
    return case


def _gen(pkg, cfg, sd, dev, precision, **kw):
    gen = pkg.HiFiGANGenerator(**{**cfg.kwargs(), **kw}, precision=precision).eval()
    gen.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()})
    return gen.to(dev)


def _check_items(gen, case, scale, precision, dev):
    """Ragged batch: each item bitwise its solo run and within ATOL of its oracle; returns the
    largest error."""
    refs = case["ref"][scale, "bf16" if precision == "bf16w" else "fp32"]
    worst = 0.0
    with torch.no_grad():
        out = gen(case["mel"].to(dev), lengths=LENS)
        for b, n in enumerate(LENS):
            solo = gen(case["mel"][b:b + 1, :, :n].contiguous().to(dev))
            m = solo.shape[-1]
            assert m == refs[b].shape[-1] == n * 256
            assert torch.equal(out[b:b + 1, :, :m], solo), (precision, b)
            assert not out[b, :, m:].any()
            err = (solo.cpu() - refs[b]).abs().max().item()
            worst = max(worst, err)
            assert err < ATOL, (precision, scale, b, err)
    torch.cuda.synchronize()
    return worst, out.cpu()


@pytest.mark.parametrize("scale,precision", [(1, "fp32"), (1, "f16x3"), (1, "bf16x3"),
                                             (1, "bf16w"), (2, "fp32"), (2, "f16x3")])
def test_v3_vs_release_oracle(pkg, dev, v3, evidence, scale, precision):
    """RELEASE_V3 on [3, 80, 100] with lengths [100, 37, 2] (several windows per item at every
    stage, a length ending inside a window, an item shorter than one window): fp32, f16x3 and
    bf16x3 against the oracle on the fp32 weights, bf16w on the bf16-rounded weights; x2
    weights (max |wav| ~0.8, tanh unsaturated) in fp32 and f16x3 (bf16x3's scale limit is a
    documented property of that mode).  The split modes must have run resblock2_bf16x3."""
    gen = _gen(pkg, v3["cfg"], v3["sd"][scale], dev, precision)
    h = gen.hip_handle(dev)
    h.profile_reset()
    h.set_profiling(True)
    worst, out = _check_items(gen, v3, scale, precision, dev)
    h.set_profiling(False)
    labels = sorted(h.profile_summary())
    fused = [k for k in labels if k.startswith("resblock2_bf16x3<")]
    assert not any(k.startswith("resblock_bf16x3<") or k.startswith("mrf_thin") for k in labels)
    assert bool(fused) == (precision != "fp32"), labels
    evidence(f"release V3 x{scale} [{precision}]: max|hip - oracle| = {worst:.3e} "
             f"(max|wav| {out.abs().max().item():.2f}; {len(fused)} resblock2 instances)")


@pytest.mark.parametrize("precision", ["f16x3", "bf16x3"])
def test_resblock2_fused_matches_layer_path(pkg, dev, v3, evidence, sched, precision):
    """resblock2_bf16x3 against one launch per conv (FUSED_RB = 0) on the same ragged batch:
    the pair kernels' bars (2e-6 f16x3, 2e-5 bf16x3), and both within 1e-4 of the oracle."""
    outs = []
    for fused in ("0", "1"):
        sched("FUSED_RB", fused)
        gen = _gen(pkg, v3["cfg"], v3["sd"][1], dev, precision)
        h = gen.hip_handle(dev)
        h.profile_reset()
        h.set_profiling(True)
        _, out = _check_items(gen, v3, 1, precision, dev)
        h.set_profiling(False)
        assert any(k.startswith("resblock2_bf16x3<") for k in h.profile_summary()) == (fused == "1")
        outs.append(out)
    diff = (outs[0] - outs[1]).abs().max().item()
    evidence(f"resblock2 fused vs layer path [{precision}]: max diff {diff:.3e}")
    assert diff < (2e-5 if precision == "bf16x3" else 2e-6)


SHAPES = [(3, [1]), (3, [1, 2]), (5, [2, 6]), (7, [3, 12]), (11, [1, 3, 5])]


@pytest.mark.parametrize("precision", ["f16x3", "bf16x3", "fp32"])
@pytest.mark.parametrize("ch", [32, 64, 128])
def test_resblock2_module_shapes(pkg, dev, precision, ch):
    """ResBlock2 and MRF(resblock="2") called on their own (hfg_resblock_forward /
    hfg_mrf_forward on an MRF handle) against the oracle block, per channel count over the
    (kernel, dilations) shapes; where the whole-block table has no instance (C = 128 beyond
    k = 3) the block runs layer by layer.  x [2, C, 700], and — the standalone entry points
    take no lengths — the second item's first 130 columns as a call of their own (shorter
    than one window).  Bar: the standalone-block bar of test_gpu_stages.py, 1e-4 scaled by
    the tensor's magnitude."""
    torch.manual_seed(1000 + ch)
    x = torch.randn(2, ch, 700) * 0.5
    refs = []
    for kr, dils in SHAPES:
        rb = pkg.ResBlock2(ch, kr, tuple(dils), precision=precision).to(dev)
        sd = {"b." + k: v.detach().cpu() for k, v in rb.state_dict().items()}
        for xi in (x, x[1:, :, :130].contiguous()):
            ref = block_forward(sd, "b", xi, kr, dils, "2")
            with torch.no_grad():
                y = rb(xi.to(dev))
            err = (y.cpu() - ref).abs().max().item()
            assert err <= ATOL * max(1.0, ref.abs().max().item()), (kr, dils, xi.shape, err)
        refs.append((rb, block_forward(sd, "b", x, kr, dils, "2")))
    mrf = pkg.MRF(ch, [k for k, _ in SHAPES], [d for _, d in SHAPES], precision=precision,
                  resblock="2")
    for j, (rb, _) in enumerate(refs):
        mrf.resblocks[j].load_state_dict(rb.state_dict())
    mrf = mrf.to(dev)
    if precision != "fp32":
        fused = [mrf._handle_for(dev).packed_resblock(0, j)[0]["fused"] for j in range(len(SHAPES))]
        assert fused == ([1, 1, 0, 0, 0] if ch == 128 else [1] * 5)
    ref = sum(r for _, r in refs) / len(refs)
    with torch.no_grad():
        y = mrf(x.to(dev))
    torch.cuda.synchronize()
    err = (y.cpu() - ref).abs().max().item()
    print(f"\nMRF(resblock='2') C={ch} [{precision}]: max err {err:.2e}")
    assert err <= ATOL * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("c0,rates,kernels", [(128, [8, 8, 2, 2], [16, 16, 4, 4]),
                                              (512, [8, 8, 4], [16, 16, 8])])
def test_thin_and_wide_stages_type2(pkg, dev, S, c0, rates, kernels):
    """ResBlock2 stages outside the whole-block kernel's range: c0 = 128 with four
    upsamplers (C = 16 and 8: the mrf_thin kernels are pair-only, so these run layer by
    layer) and c0 = 512 (C = 256).  Each precision passes at 1e-4 or is refused when the
    handle is created, with a message."""
    cfg = S.ReleaseConfig(upsample_rates=rates, upsample_kernel_sizes=kernels,
                          upsample_initial_channel=c0, resblock_kernel_sizes=[3, 5, 7],
                          resblock_dilation_sizes=[[1, 2], [2, 6], [3, 12]], resblock="2")
    sd = S.random_state_dict(cfg, seed=c0)
    mel = torch.randn(2, 80, 16, generator=torch.Generator().manual_seed(c0))
    refs = {"fp32": release_forward(sd, cfg, mel), "bf16": release_forward(_bf16_weights(sd), cfg, mel)}
    ran = 0
    for precision in ("fp32", "f16x3", "bf16x3", "bf16w"):
        gen = _gen(pkg, cfg, sd, dev, precision)
        try:
            h = gen.hip_handle(dev)
        except pkg.HfgError as e:
            print(f"c0={c0} [{precision}]: refused at creation: {e}")
            assert str(e).split(":", 1)[-1].strip(), "refusal without a message"
            continue
        h.profile_reset()
        h.set_profiling(True)
        with torch.no_grad():
            out = gen(mel.to(dev))
        torch.cuda.synchronize()
        h.set_profiling(False)
        assert not any(k.startswith("mrf_thin") for k in h.profile_summary())
        err = (out.cpu() - refs["bf16" if precision == "bf16w" else "fp32"]).abs().max().item()
        print(f"c0={c0} [{precision}]: max err {err:.2e}")
        assert err < ATOL, (precision, err)
        ran += 1
    assert ran, "every precision was refused"


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_final_slope(pkg, dev, S, evidence, sched, precision):
    """final_lrelu_slope = 0.01 on the reference's V1 architecture (what a release V1 / V2
    file needs), x2 weights, T = 24: within 1e-4 of the slope-0.01 oracle and more than 1e-3
    from the slope-0.1 one; conv_post fused into the last ResBlock launch (FUSE_POST 1,
    conv_post_tail) bitwise the separate conv_post4_tanh; the LDS-staged conv_post_tanh
    (L % 4 != 0) on the same slope; 0.1 passed explicitly bitwise the default Generator."""
    from oracle import config as C, prng
    cfg = C.V1
    sd = C.make_state_dict(cfg, seed=29, scale=2.0)
    mel_np = prng.mel_input(29, (2, 80, 24))
    mel = torch.as_tensor(mel_np).to(dev)
    rel = S.ReleaseConfig(**cfg.kwargs(), resblock="1", final_lrelu_slope=0.01)
    ref01 = release_forward(sd, rel, mel_np)
    ref10 = release_forward(sd, cfg, mel_np)
    sched("RB_CONC", "0")  # keeps this small batch on the one-launch-per-ResBlock schedule
    outs = {}
    for mode in ("0", "1"):
        sched("FUSE_POST", mode)
        gen = _gen(pkg, cfg, sd, dev, precision, final_lrelu_slope=0.01)
        h = gen.hip_handle(dev)
        h.profile_reset()
        h.set_profiling(True)
        with torch.no_grad():
            outs[mode] = gen(mel).cpu()
        torch.cuda.synchronize()
        h.set_profiling(False)
        # fp32 has no whole-ResBlock launch to fuse into
        assert ("conv_post4_tanh" in h.profile_summary()) == (mode == "0" or precision == "fp32")
    assert torch.equal(outs["0"], outs["1"])
    err = (outs["1"] - ref01).abs().max().item()
    away = (outs["1"] - ref10).abs().max().item()
    evidence(f"V1 x2 final slope 0.01 [{precision}]: max|hip - oracle(0.01)| = {err:.3e}, "
             f"max|hip - oracle(0.1)| = {away:.3e}")
    assert err < ATOL
    assert away > 1e-3
    with torch.no_grad():
        a = _gen(pkg, cfg, sd, dev, precision)(mel)
        b = _gen(pkg, cfg, sd, dev, precision, final_lrelu_slope=0.1)(mel)
    assert torch.equal(a, b)
    assert (a.cpu() - ref10).abs().max().item() < ATOL
    # L = 25 T + 6 (L % 4 == 2): conv_post_tanh
    odd = C.GenConfig(upsample_rates=[5, 5], upsample_kernel_sizes=[10, 10],
                      upsample_initial_channel=64, resblock_kernel_sizes=[3],
                      resblock_dilation_sizes=[[1, 3]])
    osd = C.make_state_dict(odd, seed=31, scale=2.0)
    omel = prng.mel_input(31, (2, 80, 24))
    gen = _gen(pkg, odd, osd, dev, precision, final_lrelu_slope=0.01)
    h = gen.hip_handle(dev)
    h.set_profiling(True)
    with torch.no_grad():
        o = gen(torch.as_tensor(omel).to(dev)).cpu()
    torch.cuda.synchronize()
    h.set_profiling(False)
    assert "conv_post_tanh" in h.profile_summary()
    orel = S.ReleaseConfig(**odd.kwargs(), resblock="1", final_lrelu_slope=0.01)
    assert (o - release_forward(osd, orel, omel)).abs().max().item() < ATOL


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_streaming_v3(pkg, dev, S, precision):
    """StreamingVocoder(chunk_frames=8) over 40 frames of the V3 generator: the
    concatenated chunks are bitwise the one-shot run (the context comes from
    receptive_field_frames(), whose ResBlock2 radius is the sum of the convs' paddings)."""
    import __graft_entry__ as ge
    glue = importlib.import_module(ge.PKG_NAME + ".glue")
    cfg = S.RELEASE_V3
    gen = _gen(pkg, cfg, S.random_state_dict(cfg, seed=23), dev, precision)
    mel = torch.randn(80, 40, generator=torch.Generator().manual_seed(23)).to(dev)
    with torch.no_grad():
        ref = gen(mel[None])[0, 0]
    sv = glue.StreamingVocoder(gen, chunk_frames=8)
    rng, pieces, pos = np.random.default_rng(3), [], 0
    while pos < 40:
        n = int(rng.integers(1, 12))
        pieces.append(sv.push(mel[:, pos:pos + n]))
        pos += n
    pieces.append(sv.flush())
    out = torch.cat(pieces)
    torch.cuda.synchronize()
    assert out.shape == ref.shape == (40 * 256,)
    assert torch.equal(out, ref)
