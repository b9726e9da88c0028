"""The discriminators on the device against the float64 ATen oracle
(tests/discriminator_oracle.py): every feature map of every parity length, the kernel's tile
edges, batch independence, guard bands, ``HiFiGAN(discriminators=True).discriminate``, the
critic metrics and graph capture.

Bar: max |device - oracle64| <= 1e-4 x that map's oracle peak (the project's per-stage bar; the
fixture weights keep the maps at unit scale, test_discriminators_host.py).  Each parity test
also prints, per map, the ratio of the device error to the oracle's own float32-vs-float64
difference.

disc_conv's tile is kDiscNt = 64 output positions (h_out, w) per block on every instance
(16 MSUB rows x 64 positions, MSUB = 4, 2, 1): the tile-edge cases put the first layer of
each instance at 64 positions and just past them.
"""
import functools
import json
import os

import pytest
import torch

from conftest import GOLDEN_DIR

import disc_cases as DC
import discriminator_oracle as DO

pytestmark = pytest.mark.gpu

BAR = 1e-4
DEV = "cuda:0"


# ---- the device modules, built once ----

@pytest.fixture(scope="module")
def D(pkg):
    return pkg.discriminators


@pytest.fixture(scope="module")
def period_discs(D):
    out = {}
    for p in DC.PERIODS:
        d = D.PeriodDiscriminator(p)
        d.load_state_dict(DC.period_state(), strict=True)
        out[p] = d.to(DEV)
    return out


@pytest.fixture(scope="module")
def scale_disc(D):
    d = D.ScaleDiscriminator()
    d.load_state_dict(DC.scale_state(), strict=True)
    return d.to(DEV)


@pytest.fixture(scope="module")
def msd(D):
    m = D.MultiScaleDiscriminator()
    m.load_state_dict(DC.msd_state_dict(), strict=True)
    return m.to(DEV)


@functools.lru_cache(maxsize=None)
def _period_ref(p, T, B=1):
    x = DC.wav(T, B)
    return (DO.period_forward(DC.f64(DC.period_state()), x.double(), p),
            DO.period_forward(DC.period_state(), x, p))


@functools.lru_cache(maxsize=None)
def _scale_ref(T, seed=DC.SEED_SCALE, gain=DC.SCALE_GAINS[0], pools=0):
    x = DC.wav(T)
    sd = DC.scale_state(seed, gain)
    return (DO.scale_forward(DC.f64(sd), DO.pool(x.double(), pools)),
            DO.scale_forward(sd, DO.pool(x, pools)))


def _check_maps(got, ref64, ref32, what, evidence):
    assert len(got) == len(ref64)
    worst_rel, worst_ratio = 0.0, 0.0
    lines = []
    for i, (g, r64, r32) in enumerate(zip(got, ref64, ref32)):
        assert tuple(g.shape) == tuple(r64.shape), (what, i, g.shape, r64.shape)
        g = g.cpu().double()
        assert torch.isfinite(g).all(), f"{what} map {i}: non-finite values"
        peak = r64.abs().max().item()
        err = (g - r64).abs().max().item()
        own = (r32.double() - r64).abs().max().item()
        ratio = err / own if own > 0 else float("inf") if err > 0 else 0.0
        lines.append(f"map {i}: err/peak {err / peak:.2e} oracle32/peak {own / peak:.2e} "
                     f"ratio {ratio:.1f}")
        worst_rel = max(worst_rel, err / peak)
        worst_ratio = max(worst_ratio, ratio)
    print(what + "\n  " + "\n  ".join(lines))
    evidence(f"{what}: worst err/peak {worst_rel:.2e}, worst ratio to the oracle's own "
             f"float32 error {worst_ratio:.1f}")
    assert worst_rel <= BAR, f"{what}: {worst_rel:.3e} of the peak > {BAR}"


# ---- map parity ----

@pytest.mark.parametrize("which", range(4), ids=["T=p", "T=2p-1", "T=243p", "T=243p+1"])
@pytest.mark.parametrize("p", DC.PERIODS)
def test_period_maps(period_discs, p, which, evidence):
    T = DC.period_lengths(p)[which]
    ref64, ref32 = _period_ref(p, T)
    out, maps = period_discs[p](DC.wav(T).to(DEV))
    assert out is maps[-1]
    _check_maps(maps, ref64, ref32, f"period {p} T {T}", evidence)


@pytest.mark.parametrize("T", DC.SCALE_LENGTHS)
def test_scale_maps(scale_disc, T, evidence):
    ref64, ref32 = _scale_ref(T)
    _check_maps(scale_disc(DC.wav(T).to(DEV))[1], ref64, ref32, f"scale T {T}", evidence)


@pytest.mark.parametrize("T", DC.MSD_LENGTHS)
def test_msd_maps(msd, T, evidence):
    outs, feats = msd(DC.wav(T).to(DEV))
    assert len(outs) == len(feats) == 3
    for i in range(3):
        ref64, ref32 = _scale_ref(T, DC.SEED_MSD[i], DC.MSD_ENTRY_GAINS[i], i)
        _check_maps(feats[i], ref64, ref32, f"msd scale {i} T {T}", evidence)


def test_period_tile_edge_msub4(period_discs, evidence):
    """disc_conv_x3<4> (64 rows x 64 positions), first on convs.1 of a period
    discriminator: period 2 at T = 560 gives it 32 x 2 = 64 positions (one full tile), T = 578
    gives 33 x 2 = 66 (a second tile of two)."""
    for T, h2 in ((560, 32), (578, 33)):
        ref64, ref32 = _period_ref(2, T)
        assert ref64[1].shape[2] == h2
        _check_maps(period_discs[2](DC.wav(T).to(DEV))[1], ref64, ref32,
                    f"period 2 T {T} (tile edge, MSUB 4)", evidence)


@pytest.mark.parametrize("T,layer,msub", [(128, 1, 2), (129, 1, 2), (255, 2, 1)])
def test_scale_tile_edges(scale_disc, T, layer, msub, evidence):
    """disc_conv_x3<2> (32 x 64) runs convs.1 (groups of 32 -> 32): T = 128 gives it 64
    positions, T = 129 gives 65.  disc_conv_x3<1> (16 x 64) runs convs.2 (8 -> 16): T = 255
    gives it 64 positions; T = 257 (65, the other side) is test_scale_maps's."""
    ref64, ref32 = _scale_ref(T)
    assert ref64[layer].shape[2] in (64, 65)
    _check_maps(scale_disc(DC.wav(T).to(DEV))[1], ref64, ref32,
                f"scale T {T} (tile edge, MSUB {msub})", evidence)


# ---- batch independence ----

def test_batch_items_are_their_solo_runs(period_discs, scale_disc):
    for disc, T in ((period_discs[3], 730), (period_discs[11], 100), (scale_disc, 257)):
        x = DC.wav(T, 3).to(DEV)
        assert not torch.equal(x[0], x[1])
        batch = disc(x)[1]
        for b in range(3):
            solo = disc(x[b:b + 1])[1]
            for i, (m, s) in enumerate(zip(batch, solo)):
                assert torch.equal(m[b:b + 1], s), f"T {T} item {b} map {i}"


# ---- guards ----

def _banded(t, band=64):
    """t inside NaN bands: (the whole buffer, the view)."""
    buf = torch.full((t.numel() + 2 * band,), float("nan"), device=DEV)
    view = buf[band:band + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def _bands_intact(buf, n, band=64):
    return bool(torch.isnan(buf[:band]).all() and torch.isnan(buf[band + n:]).all())


@pytest.mark.parametrize("kind,T", [("period", 2674), ("period", 21), ("scale", 257)])
def test_guard_bands(period_discs, msd, kind, T):
    """NaN bands around wav, every map and the workspace: nothing outside is written, and
    nothing outside [0, T) is read (the reflect pad, the zero padding and the pooling's padding
    included): the maps are bitwise those of the plain call."""
    disc = period_discs[11] if kind == "period" else msd.discriminators[2]
    B = 2
    x = DC.wav(T, B).to(DEV)
    plain = disc(x)[1]
    h = disc.hip_handle(DEV)
    xbuf, xv = _banded(x)
    bufs = [_banded(torch.zeros_like(m)) for m in plain]
    ws_bytes = h.workspace_bytes(B, T)
    wsbuf = torch.full((ws_bytes // 4 + 128,), float("nan"), device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    h.forward(xv.data_ptr(), B, T, [v.data_ptr() for _, v in bufs], wsbuf[64:].data_ptr(),
              ws_bytes, stream)
    torch.cuda.synchronize()
    assert _bands_intact(xbuf, x.numel())
    assert torch.isnan(wsbuf[:64]).all() and torch.isnan(wsbuf[64 + (ws_bytes + 3) // 4:]).all()
    for i, ((buf, v), m) in enumerate(zip(bufs, plain)):
        assert _bands_intact(buf, m.numel()), f"map {i}: band written"
        assert torch.equal(v, m), f"map {i} differs with NaN around the inputs"
    # the sums: bands around sums and the reduction's workspace
    fake = [_banded(0.5 * m)[1] for m in plain]
    sums = torch.full((B * len(plain) + 16,), float("nan"), dtype=torch.float64, device=DEV)
    fm_bytes = h.fm_workspace_bytes(B)
    fm_ws = torch.full((fm_bytes // 8 + 16,), float("nan"), dtype=torch.float64, device=DEV)
    h.fm_sums(B, T, [v.data_ptr() for _, v in bufs], [f.data_ptr() for f in fake],
              sums[8:].data_ptr(), fm_ws[8:].data_ptr(), fm_bytes, stream)
    torch.cuda.synchronize()
    assert torch.isnan(sums[:8]).all() and torch.isnan(sums[8 + B * len(plain):]).all()
    assert torch.isnan(fm_ws[:8]).all() and torch.isnan(fm_ws[8 + fm_bytes // 8:]).all()
    got = sums[8:8 + B * len(plain)].view(B, len(plain))
    want = torch.stack([torch.stack([(0.5 * m[b].double()).abs().sum() for m in plain])
                        for b in range(B)])
    assert torch.allclose(got, want, rtol=1e-12, atol=0)


def test_input_rules(period_discs):
    x = DC.wav(30).to(DEV).requires_grad_(True)
    with pytest.raises(NotImplementedError):
        period_discs[3](x)
    with torch.no_grad():
        period_discs[3](x)
    with pytest.raises(RuntimeError, match="reflect pad"):
        period_discs[11](DC.wav(5).to(DEV))


# ---- HiFiGAN(discriminators=True) ----

def test_hifigan_discriminate(pkg, evidence):
    """The 8-tuple at T = 257 with the oracle's shapes, weights from a seeded torch.Generator
    (the keyed PRNG is too slow for 70 M parameters); two spot maps per discriminator at the
    bar; the 2B batch inside is bitwise the two separate calls."""
    m = pkg.HiFiGAN(discriminators=True)
    gen = torch.Generator().manual_seed(1234)
    sd = m.state_dict()
    new = {}
    for k, v in sd.items():
        if not k.startswith(("msd.", "mpd.")):
            new[k] = v
        elif k.endswith("weight_g"):
            new[k] = v * 2.0
        else:
            new[k] = (torch.rand(v.shape, generator=gen) * 2 - 1) * v.abs().max()
    for k in [k for k in new if k.endswith("weight_g")]:
        vv = new[k[:-1] + "v"]
        new[k] = 2.0 * vv.reshape(vv.shape[0], -1).norm(dim=1).reshape(new[k].shape)
    m.load_state_dict(new, strict=True)
    m = m.to(DEV)
    real, fake = DC.loss_pair(257)
    out = m.discriminate(real.to(DEV), fake.to(DEV))
    assert len(out) == 8
    assert [len(o) for o in out] == [3, 3, 3, 3, 5, 5, 5, 5]
    sub = lambda pre, i: {k[len(f"{pre}.discriminators.{i}."):]: v.double() for k, v in new.items()
                          if k.startswith(f"{pre}.discriminators.{i}.")}
    refs = ([DO.scale_forward(sub("msd", i), DO.pool(w.double(), i)) for i in range(3)]
            for w in (real, fake))
    ref_real_s, ref_fake_s = list(refs)
    ref_real_p, ref_fake_p = ([DO.period_forward(sub("mpd", i), w.double(), p)
                               for i, p in enumerate(DO.PERIODS)] for w in (real, fake))
    worst = 0.0
    for outs, feats, ref in ((out[0], out[1], ref_real_s), (out[2], out[3], ref_fake_s),
                             (out[4], out[5], ref_real_p), (out[6], out[7], ref_fake_p)):
        for d, (o, f, r) in enumerate(zip(outs, feats, ref)):
            assert [tuple(t.shape) for t in f] == [tuple(t.shape) for t in r]
            assert tuple(o.shape) == tuple(r[-1].shape) and torch.equal(o, f[-1])
            for i in (2, len(r) - 1):
                err = (f[i].cpu().double() - r[i]).abs().max().item() / r[i].abs().max().item()
                worst = max(worst, err)
                assert err <= BAR, f"discriminator {d} map {i}: {err:.3e}"
    evidence(f"discriminate spot maps: worst err/peak {worst:.2e}")
    sep_real = m.msd(real.to(DEV))[1] + m.mpd(real.to(DEV))[1]
    sep_fake = m.msd(fake.to(DEV))[1] + m.mpd(fake.to(DEV))[1]
    for a, b in zip(out[1] + out[5], sep_real):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    for a, b in zip(out[3] + out[7], sep_fake):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- the critic metrics ----

@pytest.fixture(scope="module")
def critics(D, msd):
    mpd = D.MultiPeriodDiscriminator()
    mpd.load_state_dict({f"discriminators.{i}.{k}": v for i, s in enumerate(DC.SEED_MPD)
                         for k, v in DC.period_state(s).items()}, strict=True)
    return [msd, mpd.to(DEV)]


@functools.lru_cache(maxsize=None)
def _loss_ref64():
    real, fake = (t.double() for t in DC.loss_pair())
    s = [DC.f64(sd) for sd in DC.msd_states()]
    p = [DC.f64(DC.period_state(seed)) for seed in DC.SEED_MPD]
    rm = DO.msd_forward(s, real) + DO.mpd_forward(p, real)
    fm = DO.msd_forward(s, fake) + DO.mpd_forward(p, fake)
    total, per = DO.feature_matching_loss(rm, fm)
    ro, fo = [m[-1] for m in rm], [m[-1] for m in fm]
    return (float(total), [float(v) for v in per], float(DO.discriminator_loss(ro, fo)),
            float(DO.generator_adversarial_loss(fo)))


def test_feature_matching_and_scores_match_the_oracle(pkg, critics, evidence):
    total, per, d_loss, g_adv = _loss_ref64()
    with open(os.path.join(GOLDEN_DIR, "disc_loss_ref.json")) as f:
        ref = json.load(f)
    assert abs(total - ref["feature_matching"]) <= 1e-5 * total   # the reference's float32
    real, fake = (t.to(DEV) for t in DC.loss_pair())
    fm = pkg.metrics.feature_matching(critics, real, fake)
    assert fm.total.dtype == torch.float64 and fm.total.is_cuda
    rel = lambda a, b: abs(a - b) / abs(b)
    errs = [rel(fm.total.item(), total)] + [rel(g, w) for g, w in
                                            zip(fm.per_discriminator.tolist(), per)]
    sr = pkg.metrics.discriminator_scores(critics, real)
    sf = pkg.metrics.discriminator_scores(critics, fake)
    errs += [rel(sr.discriminator_loss(sr, sf).item(), d_loss),
             rel(sf.generator_adversarial.item(), g_adv)]
    evidence(f"critic metrics vs the float64 oracle: worst relative difference {max(errs):.2e}")
    assert max(errs) <= 1e-5, errs
    assert rel(fm.per_item[0].item(), total) <= 1e-5      # B = 1: the item is the batch


def test_feature_matching_is_deterministic_and_per_item(pkg, critics):
    real = DC.wav(257, 3).to(DEV)
    fake = 0.9 * real + 0.01 * DC.wav(257, 3, seed=77).to(DEV)
    a = pkg.metrics.feature_matching(critics, real, fake)
    b = pkg.metrics.feature_matching(critics, real, fake)
    assert torch.equal(a.per_item, b.per_item) and torch.equal(a.total, b.total)
    assert torch.equal(a.per_discriminator, b.per_discriminator)
    assert a.per_item.shape == (3,)
    for i in range(3):
        solo = pkg.metrics.feature_matching(critics, real[i:i + 1], fake[i:i + 1])
        assert torch.equal(solo.per_item[0], a.per_item[i]), i
    same = pkg.metrics.feature_matching(critics, real, real)
    assert same.total.item() == 0.0 and (same.per_item == 0).all()


def test_critic_distance(pkg, critics):
    import importlib
    from oracle import config as C, prng
    glue = importlib.import_module("tts_sambert_hifigan_amd.glue")
    cfg = C.V1
    gen = pkg.HiFiGANGenerator(**cfg.kwargs()).eval()
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in C.make_state_dict(cfg, 11).items()})
    gen = gen.to(DEV)
    mel = torch.from_numpy(prng.mel_input(11, (1, cfg.n_mels, 4))).to(DEV)
    real = DC.wav(1100).to(DEV)
    fm = glue.critic_distance(gen, critics[1], mel, real)
    n = fm.wav_fake.shape[-1]
    assert n == 1024
    want = pkg.metrics.feature_matching(critics[1], real[..., :n], fm.wav_fake)
    assert torch.equal(fm.total, want.total) and fm.total.item() > 0


# ---- capture ----

def test_capture_replays_bitwise(period_discs):
    """One torch.cuda.graph capture of a PeriodDiscriminator forward plus the feature-matching
    sums, all on one stream, replayed on new input: bitwise the eager result."""
    disc, T, B = period_discs[5], 1216, 2
    h = disc.hip_handle(DEV)
    shapes = h.map_shapes(T)
    x = torch.zeros(2 * B, 1, T, device=DEV)
    maps = [torch.empty((2 * B,) + s, device=DEV) for s in shapes]
    ws = torch.empty(max(h.workspace_bytes(2 * B, T), 16), dtype=torch.uint8, device=DEV)
    sums = torch.zeros(B, len(maps), dtype=torch.float64, device=DEV)
    fm_ws = torch.empty(h.fm_workspace_bytes(B), dtype=torch.uint8, device=DEV)

    def work():
        s = torch.cuda.current_stream().cuda_stream
        h.forward(x.data_ptr(), 2 * B, T, [m.data_ptr() for m in maps], ws.data_ptr(), ws.numel(),
                  s)
        h.fm_sums(B, T, [m.data_ptr() for m in maps], [m[B:].data_ptr() for m in maps],
                  sums.data_ptr(), fm_ws.data_ptr(), fm_ws.numel(), s)

    x.copy_(DC.wav(T, 2 * B, seed=3).to(DEV))
    work()                                  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        work()
    new = DC.wav(T, 2 * B, seed=9).to(DEV)
    x.copy_(new)
    g.replay()
    torch.cuda.synchronize()
    got_maps, got_sums = [m.clone() for m in maps], sums.clone()
    eager = disc(new)[1]
    for i, (a, b) in enumerate(zip(got_maps, eager)):
        assert torch.equal(a, b), f"map {i}"
    work()
    torch.cuda.synchronize()
    assert torch.equal(got_sums, sums) and (got_sums > 0).all()
