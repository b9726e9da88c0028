"""Window seams and sequence ends, on the CPU (tests/seam_cases.py): every probe handle runs the
launch it exists for, its length classes are realised from the plan dump, the probe weights
make a one-column halo error, a shifted window origin, a missing end-of-sequence mask and
swapped dilations of the float64 restatement move the output by at least 10 x the widest bar
(where default-init weights move it by less than the bars: recorded, not asserted), and the
standalone probes are exact in every number format the kernels use."""
import numpy as np
import pytest

import seam_cases as S
from oracle import hifigan_np64 as N
from oracle import prng

NAMES = [c.name for c in S.CASES]
WINDOWED = [c.name for c in S.CASES if c.launch != "layer"]
BLOCKS = [c.name for c in S.CASES if c.blk.j >= 0]


def _rb0(plan):
    return plan["stages"][0]["rbs"][0]


# ----------------------------------------------------------------------------------------
# coverage: each handle runs its launch, each length class exists
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_case_runs_the_launch_it_exists_for(pkg, name):
    case = S.BY_NAME[name]
    blk = case.blk
    p16, p32 = S.host_plan(pkg, blk, "f16x3"), S.host_plan(pkg, blk, "fp32")
    st = p16["stages"][0]
    assert st["C"] == blk.channels
    # the fp32 precision has no whole-block launch; the thin kernel serves it too
    assert not any(rb["fused"] for rb in p32["stages"][0]["rbs"])
    geo = ("fused", "nwin", "halo", "W", "split", "parts")
    for prec in S.SPLIT_PRECISIONS[1:]:   # one geometry for the three split precisions
        other = S.host_plan(pkg, blk, prec)["stages"][0]
        assert (other["thin"], other["thin_mfma"]) == (st["thin"], st["thin_mfma"])
        assert [{k: rb.get(k) for k in geo} for rb in other["rbs"]] == \
            [{k: rb.get(k) for k in geo} for rb in st["rbs"]], prec
    if case.launch in ("thin", "thin_mfma"):
        assert st["thin"] == 1 and p32["stages"][0]["thin"] == 1
        assert st["thin_mfma"] == (case.launch == "thin_mfma") and not p32["stages"][0]["thin_mfma"]
        halos = [sum(S.radius(k, d) for _, k, d, _ in S.case_convs(blk, j)) for j in blk.blocks]
        assert st["thin_halo"] == halos   # a thin window pays every conv's radius
        return
    rb = _rb0(p16)
    convs = S.case_convs(blk, blk.j)
    rad = [S.radius(k, d) for _, k, d, _ in convs]
    assert st["thin"] == 0
    if case.launch == "layer":
        assert rb["fused"] == 0
        L = p16["layers"][0]
        assert L["prec"] == 1 and L["small"][0] == 4, L
        if blk.channels >= 256:   # A fragments in registers (kernels.h kAregTile / kAregTallTile)
            assert L["tile"] in (5, 6) and S.BF16X3_TILES[L["tile"]][6], L
        return
    assert rb["fused"] == 1 and rb["nwin"] == case.nwin and rb["kt"] == blk.kernels[blk.j]
    # halo = sum of the radii - r[0]; W = (nwin - 2 halo) & ~3  (plan.cpp RbConvs::halo, window_width)
    assert rb["halo"] == sum(rad) - rad[0]
    assert rb["W"] == S.window_width(rb["nwin"], rb["halo"]) == (rb["nwin"] - 2 * rb["halo"]) & ~3
    assert len(rb["convs"]) == len(convs) == len(p16["layers"])
    assert bool(rb["split"]) == (case.launch == "split")
    if rb["split"]:
        s = rb["split"]
        assert s % 2 == 0 and 0 < s < len(convs)
        h0, h1 = sum(rad[:s]) - rad[0], sum(rad[s:]) - rad[s]
        assert rb["parts"] == [h0, h1, S.window_width(rb["nwin"], h0), S.window_width(rb["nwin"], h1)]
    if case.launch == "rb2":
        assert all(".convs." in L["mod"] for L in p16["layers"]) and len(convs) == len(blk.dilations[blk.j])


@pytest.mark.parametrize("name", [c.name for c in S.CASES if c.launch in ("fused", "split", "rb2")])
def test_schedule_knobs_move_the_case_off_its_launch(pkg, sched, name):
    """FUSED_RB 0 runs every whole-block case layer by layer, RB_SPLIT 0 a split one as one
    launch of the whole window: the knob sets of the GPU test select different kernels."""
    blk = S.BY_NAME[name].blk
    S.windows(pkg, name)   # (the default schedule's geometry, cached before any override)
    sched("FUSED_RB", 0)
    assert _rb0(S.host_plan(pkg, blk))["fused"] == 0
    sched("FUSED_RB", 1)
    sched("RB_SPLIT", 0)
    rb = _rb0(S.host_plan(pkg, blk))
    whole = next(w for w in S.windows(pkg, name) if w.tag == "whole")
    assert rb["fused"] == 1 and rb["split"] == 0 and (rb["W"], rb["halo"]) == (whole.W, whole.halo)


@pytest.mark.parametrize("name", NAMES)
def test_knob_sets_are_fixed_by_the_launch(name):
    case = S.BY_NAME[name]
    want = {"fused": 3, "split": 3, "rb2": 2, "thin": 1, "thin_mfma": 1, "layer": 2}[case.launch]
    sets = S.knob_sets(case)
    assert len(sets) == want and all(k in ("FUSED_RB", "RB_SPLIT", "SMALL_TILE") for s in sets for k in s)
    assert (sets[0] == {}) == (case.launch != "layer")


@pytest.mark.parametrize("name", NAMES)
def test_length_classes_are_realised(pkg, name, evidence):
    """Every class of every launch geometry of the handle is one of the case's lengths (the
    classes that are no length, halo = 0 and r_max = 0 of a layer launch, aside), the classes
    of a windowed launch are at least 14 distinct lengths, and all four residues of L mod 4
    appear."""
    ws, Ls = S.windows(pkg, name), S.lengths(pkg, name)
    cap = S.max_length(pkg, name)
    assert ws and {L % 4 for L in Ls} == {0, 1, 2, 3}
    assert max(Ls) <= cap and min(Ls) == 1
    tags = [w.tag for w in ws]
    assert len(set(tags)) == len(tags)
    for w in ws:
        cls = S.length_classes(w)
        assert list(cls) == list(S.CLASSES)
        inside = {c: L for c, L in cls.items() if 1 <= L <= cap}
        assert set(inside.values()) <= set(Ls)
        # one, two and three windows, and the seam itself, are always within the cap
        for c in ("1", "W-1", "W", "W+1", "2W-1", "2W", "2W+1", "2W+halo+2"):
            assert c in inside, (w, c)
        if w.windowed:
            # (a halo of 2, ResBlock2 k = 3, makes W + 1 = W + halo - 1 and two more pairs coincide)
            assert len(inside) == len(S.CLASSES) and len(set(inside.values())) >= 14, (w, inside)
            assert 0 < w.r_max and 0 < w.halo < w.W and w.W + 2 * w.halo <= w.nwin
    evidence(f"{len(Ls)} lengths in [1, {max(Ls)}] from " +
             ", ".join(f"{w.tag} (W {w.W}, halo {w.halo}, nwin {w.nwin})" for w in ws))


# ----------------------------------------------------------------------------------------
# the probes resolve seam errors; default-init weights do not
# ----------------------------------------------------------------------------------------
def _bar(ref):
    return S.stage_bar(S.WIDEST, float(np.abs(ref).max()), 0.0)


def _moves(muts, ref):
    """{mutant: (max move, columns that moved)}; the exact windows must reproduce ref."""
    out = {}
    for m in S.MUTANTS:
        d = np.abs(muts[m][0] - ref)
        out[m] = (float(d.max()), d.max(axis=(0, 1)) > 1e-9 * max(1.0, float(np.abs(ref).max())))
    return out


@pytest.mark.parametrize("name", WINDOWED)
def test_probes_resolve_seam_mutants(pkg, name, evidence):
    """On the float64 restatement alone, per windowed launch geometry of the case: the windows
    with the plan's halo reproduce the unwindowed block exactly; each mutant (a) - (d) moves the
    output by >= 10 x the bf16x3 stage bar, in the columns where it should."""
    blk = S.BY_NAME[name].blk
    worst = None
    for w in S.windows(pkg, name):
        if not w.windowed:
            continue
        L = S.mutant_length(w, S.max_length(pkg, name))
        x, ref = S.probe_ref(name, L)
        muts = S.mutants(blk, w, x)
        if blk.j >= 0:
            assert np.array_equal(muts["exact"][0], ref), (name, w.tag)
        else:   # the MRF's division by n_res
            assert np.abs(muts["exact"][0] - ref).max() <= 1e-12 * np.abs(ref).max()
        bar = _bar(ref)
        for m, (moved, cols) in _moves(muts, ref).items():
            ratio = moved / bar
            if worst is None or ratio < worst[0]:
                worst = (ratio, w.tag, m, moved, bar, L)
            assert ratio >= 10.0, (name, w.tag, m, moved, bar)
            allowed = muts[m][1]
            assert cols.any() and not (cols & ~allowed).any(), \
                (name, w.tag, m, np.flatnonzero(cols & ~allowed)[:8], S.seams(w, L))
    evidence(f"smallest mutant move / bf16x3 bar = {worst[0]:.3g} ({worst[1]}, {worst[2]}: moved "
             f"{worst[3]:.3g}, bar {worst[4]:.3g}, L = {worst[5]})")


@pytest.mark.parametrize("name", [n for n in WINDOWED if S.BY_NAME[n].blk.resblock == "1"])
def test_default_scale_moves_are_recorded(pkg, name, evidence):
    """The same mutants on default-init weights and a 0.5 randn input: the evidence for why the
    probe tests exist.  The halo and dilation mutants of the k = 7 / 11 blocks stay under the
    random-data bars (1e-4 max(1, |ref|) standalone, 4e-5 max|ref| for bf16x3 stages); only
    finiteness is asserted."""
    blk = S.BY_NAME[name].blk
    sd = S.default_state(blk)
    rows = []
    for w in S.windows(pkg, name):
        if not w.windowed:
            continue
        L = S.mutant_length(w, S.max_length(pkg, name))
        x = prng.normal(blk.seed, f"x{L}", (2, blk.channels, L), 0.5)
        ref = S.reference(blk, x, sd)
        muts = S.mutants(blk, w, x, sd)
        assert np.abs(muts["exact"][0] - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
        mv = _moves(muts, ref)
        assert all(np.isfinite(v) for v, _ in mv.values())
        rows.append(f"{w.tag} max|ref| {np.abs(ref).max():.2f}, bf16x3 bar {_bar(ref):.1e}: " +
                    ", ".join(f"{m} {v:.1e}" for m, (v, _) in mv.items()))
    evidence("default-init moves: " + "; ".join(rows))


@pytest.mark.parametrize("name", BLOCKS)
def test_standalone_probe_values_are_exact_in_every_format(pkg, name):
    """Every float64 reference value of a ResBlock / ResBlock2 probe, and every intermediate,
    is a non-negative integer < 2^16: bf16 hi + lo and scaled-f16 hi + lo hold it exactly, fp32
    sums of such values are exact, leaky_relu is the identity."""
    blk = S.BY_NAME[name].blk
    Ls = S.lengths(pkg, name)
    # the largest value the chain can reach (every conv: two inputs + a bias of 1) bounds every
    # intermediate too: a pair maps a maximum m to m + 2 (2 m + 1) + 1, a ResBlock2 conv to 3 m + 1
    top = 3
    for _ in blk.dilations[blk.j]:
        top = 3 * top + 1 if blk.resblock == "2" else 5 * top + 3
    assert top < 2 ** 16
    for L in (Ls[0], Ls[len(Ls) // 2], Ls[-1]):
        x, ref = S.probe_ref(name, L)
        assert set(np.unique(x)) <= {0.0, 1.0, 2.0, 3.0}
        assert ref.min() >= 0 and ref.max() <= top and np.array_equal(ref, np.round(ref))
    sd = S.probe_state(blk)
    for k, v in sd.items():
        assert set(np.unique(v)) <= {0.0, 1.0}, k


def test_float64_entries_agree_with_the_generator_restatement():
    """oracle/hifigan_np64.py: mrf_forward on the ups tap reproduces the Generator's mrfs tap."""
    from oracle import config as C
    sd = C.make_state_dict(C.V2STAR, seed=3)
    taps = {}
    N.generator_forward(sd, C.V2STAR, prng.mel_input(3, (1, 80, 3)),
                        tap=lambda n, t: taps.__setitem__(n, t.copy()))
    f = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    for i in range(4):
        got = N.mrf_forward(f, f"mrfs.{i}.", taps[f"ups.{i}"], C.V2STAR.resblock_kernel_sizes,
                            C.V2STAR.resblock_dilation_sizes)
        assert np.array_equal(got, taps[f"mrfs.{i}"]), i


# ----------------------------------------------------------------------------------------
# generators with a probe tail
# ----------------------------------------------------------------------------------------
def test_generator_tails_run_their_launches(pkg, evidence):
    """V1's last MRF ends in the fused conv_post launch (FUSE_POST 0: its own kernel), V2*'s
    last stage is thin; the ragged items' last-stage lengths 256 n fall into different window
    counts of every launch of the stage."""
    ws = S.gen_tail_windows(pkg, "v1")
    post = [w for w in ws if w.tag == "post"]
    assert len(post) == 1 and post[0].j == 2
    src = next(w for w in ws if w.j == 2 and w.tag in ("part1", "whole"))
    assert post[0].halo == src.halo + 3 and post[0].W == (post[0].nwin - 2 * post[0].halo) & ~3
    assert {w.tag for w in ws} >= {"whole", "part0", "part1", "post"}
    (thin,) = S.gen_tail_windows(pkg, "v2star")
    assert thin.tag == "thin" and thin.halo == 51
    lens = [256 * n for n in S.GEN_LENS]
    for w in ws + [thin]:
        counts = {-(-L // w.W) for L in lens}
        assert len(counts) >= 2 and max(lens) <= 2 * w.nwin + 64, (w, counts)
        # an end inside a window, past a seam by more and by less than the halo
        assert any(0 < L % w.W for L in lens), w
    evidence("last-stage lengths " + str(lens) + " against " +
             ", ".join(f"{w.tag} W {w.W} halo {w.halo}" for w in ws + [thin]))


def _gen_tail(name):
    """(x = ups tap, ref stage, ref wav, f, blk, post weights) in float64."""
    cfg = S.GEN_CONFIGS[name]
    last = len(cfg.upsample_rates) - 1
    r64, _ = S.gen_refs(name)
    sd = S.gen_state(name)
    pw, pb = sd["conv_post.weight"].astype(np.float64), sd["conv_post.bias"].astype(np.float64)
    return r64[f"ups.{last}"], r64[f"mrfs.{last}"], r64["wav"], S.probe_state(S.gen_blk(name), S.GEN_BIAS), \
        S.gen_blk(name), pw, pb


@pytest.mark.parametrize("name", ["v1", "v2star"])
def test_generator_probes_resolve_seam_mutants(pkg, name, evidence):
    """The Generator probes: each mutant of each launch of the last stage moves the mrfs tap by
    >= 10 x its bf16x3 stage bar and the wav by >= 10 x 1e-4; V1's fused conv_post launch is
    restated with conv_post inside the window."""
    x, stage, wav, f, blk, pw, pb = _gen_tail(name)
    n_res = len(blk.kernels)
    _, r32 = S.gen_refs(name)
    last = len(S.GEN_CONFIGS[name].upsample_rates) - 1
    cond = float(np.abs(r32[f"mrfs.{last}"] - stage).max())
    bar = S.stage_bar(S.WIDEST, float(np.abs(stage).max()), cond)
    assert np.abs(wav).max() < 0.8, "tanh does not saturate"
    blocks = [N.resblock_forward(f, f"resblocks.{j}", x, blk.kernels[j], blk.dilations[j]) for j in range(n_res)]
    assert np.abs(sum(blocks) / n_res - stage).max() <= 1e-12 * np.abs(stage).max()
    worst_s = worst_w = None
    for w in S.gen_tail_windows(pkg, name):
        if w.tag == "post":
            continue
        muts = S.mutants(blk, w, x, f)
        for m in S.MUTANTS:
            got = muts[m][0] if w.j < 0 else (sum(blocks) - blocks[w.j] + muts[m][0]) / n_res
            ds = float(np.abs(got - stage).max())
            dw = float(np.abs(np.tanh(N.conv1d(N.lrelu(got), pw, pb, 3, 1)) - wav).max())
            worst_s = min(worst_s or (np.inf,), (ds / bar, w.tag, m))
            worst_w = min(worst_w or (np.inf,), (dw / S.ATOL, w.tag, m))
            assert ds >= 10 * bar and dw >= 10 * S.ATOL, (name, w.tag, m, ds, bar, dw)
    line = (f"smallest stage move / bf16x3 bar = {worst_s[0]:.3g} ({worst_s[1]}, {worst_s[2]}); "
            f"smallest wav move / 1e-4 = {worst_w[0]:.3g} ({worst_w[1]}, {worst_w[2]})")
    post = [w for w in S.gen_tail_windows(pkg, name) if w.tag == "post"]
    if post:
        (w,) = post
        convs = S.case_convs(blk, w.j)
        L = x.shape[-1]
        xin = S.windowed_forward(f, convs[:w.conv0], x, L, L, 0, True) if w.conv0 else x
        others = sum(blocks) - blocks[w.j]
        n = w.conv1 - w.conv0

        def run(**kw):
            return S.windowed_forward(f, convs[w.conv0:w.conv1], xin, L, w.W, w.halo, True,
                                      post=(others, n_res, pw, pb), **kw)

        assert np.abs(run() - wav).max() <= 1e-12
        worst_p = (np.inf,)
        for m, kw in (("a:left", dict(short=(1, 0))), ("a:right", dict(short=(0, 1))),
                      ("b:origin", dict(shift=1)), ("c:all", dict(unmasked=tuple(range(1, n)))),
                      ("c:last", dict(unmasked=(n - 1,)))):
            dw = float(np.abs(run(**kw) - wav).max())
            worst_p = min(worst_p, (dw / S.ATOL, m))
            assert dw >= 10 * S.ATOL, (m, dw)
        line += f"; fused conv_post launch: smallest wav move / 1e-4 = {worst_p[0]:.3g} ({worst_p[1]})"
    evidence(line)
