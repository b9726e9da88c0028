"""Tap geometry at the planner's limits, on the CPU (tests/tap_cases.py): every case is placed by
the f16x3 and the fp32 plan where it says, its limit quantity touches the constant it names, one
step past each refusing limit is refused at creation with a message that names the module and
the span, every probe value is an integer below 2^16, and the probes resolve what they are for:
mutants of the float64 restatement (project code is never made wrong) move the reference by at
least 100 x the bar the GPU test asserts."""
import operator

import numpy as np
import pytest
import torch

import seam_cases as S
import tap_cases as T

NAMES = [c.name for c in T.CASES]
REL = {"==": operator.eq, "<": operator.lt, ">": operator.gt}
MIN_RATIO = 100.0


# ----------------------------------------------------------------------------------------
# 1. case pinning and refusals
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_case_sits_where_it_says(pkg, name, evidence):
    case = T.BY_NAME[name]
    blk = case.blk
    move = f"{name} no longer sits on its limit ({case.why}): move the case"
    sig = {p: T.signature(S.host_plan(pkg, blk, p)) for p in S.PRECISIONS}
    assert sig["f16x3"] == case.pin16, (move, sig["f16x3"])
    assert sig["fp32"] == case.pin32, (move, sig["fp32"])
    assert sig["bf16x3"] == sig["bf16w"] == sig["f16x3"], "one geometry for the split precisions"
    kind = case.pin16[0]
    assert kind == {"fused": "rb", "split": "rb", "rb2": "rb", "thin": "thin", "thin_mfma": "thin",
                    "layer": "layer"}[case.launch]
    assert case.pin32[0] != "rb", "the fp32 precision has no whole-block launch"
    convs = T.all_convs(blk)
    assert len(case.pin16[-1]) == len(case.pin32[-1]) == len(convs)
    rad = [S.radius(k, d) for _, k, d, _ in convs]
    if kind == "rb":
        _, kt, nwin, halo, W, split, parts, _ = case.pin16
        assert kt == blk.kernels[0] and bool(split) == (case.launch == "split")
        assert halo == sum(rad) - rad[0] and W == S.window_width(nwin, halo) > 0
        assert max(rad) <= T.LIMITS["rb_marg(64, 256)" if (blk.channels, nwin) == (64, 256) else
                                    "rb_marg(128, 256)" if blk.channels == 128 else
                                    "rb_marg(C <= 64, 512)"]
        assert len(convs) <= T.LIMITS["kRbMaxConv"] and (not case.nwin or case.nwin == nwin)
        if split:
            h0, h1 = sum(rad[:split]) - rad[0], sum(rad[split:]) - rad[split]
            assert parts == (h0, h1, S.window_width(nwin, h0), S.window_width(nwin, h1))
    elif kind == "thin":
        _, mfma, halos, _ = case.pin16
        assert bool(mfma) == (case.launch == "thin_mfma") and halos == (sum(rad),) == case.pin32[2]
        lib = pkg.load_library()
        nwin = lib.hfg_debug_thin_window(blk.channels, 0)
        assert nwin - 2 * sum(rad) >= nwin // 4 and max(rad) <= T.LIMITS["kThinMarg"]
        assert not mfma or lib.hfg_debug_thin_window(blk.channels, 1) == nwin
        assert not case.nwin or case.nwin == nwin
    # the split-precision layer kernel runs a conv iff it is within all three of its limits
    for (prec, tile, _, _), (_, k, d, _) in zip(case.pin16[-1], convs):
        inside = (d <= T.LIMITS["kMaxDil"] and k <= T.LIMITS["bf16x3 taps"] and
                  (k - 1) * d <= T.LIMITS["kBf16x3MaxHalo"] and blk.channels >= 32)
        assert prec == int(inside), (name, k, d)
        if prec and blk.channels >= 256:   # A in registers iff the tap count has an instance
            assert (tile in (5, 6)) == (k in (3, 5, 7, 11)), (name, k, tile)
    if case.limit:
        what, rel, const = case.limit
        q = T.quantity(case, what)
        assert REL[rel](q, T.LIMITS[const]), (move, what, q, const, T.LIMITS[const])
        evidence(f"{case.launch}: {what} = {q} {rel} {const} = {T.LIMITS[const]}; f16x3 plan {case.pin16[:-1]}")
    else:
        evidence(f"{case.launch}: f16x3 plan {case.pin16[:-1]}")


def test_every_limit_has_a_case_on_it():
    """Each constant of LIMITS is touched exactly ("==") by a case, or is marked unreachable
    (rb_marg at C = 128: the one k = 3 instance cannot pass r = 16), or is stepped over from both
    sides."""
    by = {}
    for c in T.CASES:
        if c.limit:
            by.setdefault(c.limit[2], set()).add(c.limit[1])
    for c in T.UPS_CASES:
        by.setdefault(c.limit[2], set()).add(c.limit[1])
    assert set(by) | {"rb_marg(128, 256)"} == set(T.LIMITS) | set(T.UPS_LIMITS)
    for const, rels in by.items():
        assert "==" in rels or rels >= {"<", ">"}, (const, rels)


@pytest.mark.parametrize("name", [c.name for c in T.CASES if c.launch in ("fused", "split", "rb2")])
def test_knobs_move_the_case_off_its_launch(pkg, sched, name):
    case = T.BY_NAME[name]
    S.block_windows(pkg, case.blk)   # (the default schedule's geometry, cached before any override)
    sched("FUSED_RB", 0)
    assert T.signature(S.host_plan(pkg, case.blk))[0] == "layer"
    sched("FUSED_RB", 1)
    sched("RB_SPLIT", 0)
    sig = T.signature(S.host_plan(pkg, case.blk))
    assert sig[0] == "rb" and sig[5] == 0 and sig[2:5] == case.pin16[2:5]


@pytest.mark.parametrize("name", [r[0] for r in T.REFUSALS])
@pytest.mark.parametrize("precision", S.PRECISIONS)
def test_one_step_past_a_refusing_limit_is_refused_at_creation(pkg, name, precision):
    _, make, mrf, module, words = next(r for r in T.REFUSALS if r[0] == name)
    with pytest.raises(Exception) as e:
        pkg.Handle(make(pkg, precision), -1, mrf=mrf) if mrf else pkg.Handle(make(pkg, precision), -1)
    msg = str(e.value)
    assert module in msg and all(w in msg for w in words), msg


# ----------------------------------------------------------------------------------------
# 2. probe exactness and lengths
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_probe_values_are_integers_below_2_16(pkg, name, evidence):
    """Every activation of the case, at every one of its lengths, from the float64 reference:
    a non-negative integer < 2^16 (exact in bf16 hi + lo and in scaled f16 hi + lo, leaky_relu
    the identity); the weights are zeros and ones."""
    case = T.BY_NAME[name]
    Ls = S.block_lengths(pkg, case.blk)
    cap = S.block_max_length(pkg, case.blk)
    assert min(Ls) == 1 and max(Ls) <= cap and {L % 4 for L in Ls} == {0, 1, 2, 3}
    assert cap <= (S.MAX_LAYER_COLS if case.blk.channels >= 256 else 2 * 1024 + 64)
    top = 0.0
    for L in Ls:
        x, ref = T.tap_ref(pkg, name, L)
        assert set(np.unique(x)) <= ({0.0, 1.0} if case.sparse else {0.0, 1.0, 2.0, 3.0}) | {float(case.spike)}
        out, seen = T.forward64(name, x)
        assert np.array_equal(out, ref), "forward64 restates the oracle's reference"
        for t in seen:
            assert t.min() >= 0 and np.array_equal(t, np.round(t))
            top = max(top, float(t.max()))
    assert top < 2 ** 16 and (top > 0 or max(Ls) == 1)
    for k, v in T.tap_state(name).items():
        assert set(np.unique(v)) <= {0.0, 1.0}, k
    evidence(f"{len(Ls)} lengths in [1, {max(Ls)}]; largest activation {top:.0f}")


# ----------------------------------------------------------------------------------------
# 3. the probes resolve what they are for
# ----------------------------------------------------------------------------------------
def _ratios(moved, ref, rtol=S.RTOL.get):
    """{precision: move / the bar the GPU test asserts for it} (rtol: TapCase.rtol)."""
    return {p: moved / (rtol(p) * max(1.0, float(np.abs(ref).max()))) for p in S.PRECISIONS}


@pytest.mark.parametrize("name", NAMES)
def test_probes_resolve_tap_mutants(pkg, name, evidence):
    """Per case, on the float64 restatement alone: the outermost tap of its widest conv placed
    as at dilation d - 1, and per windowed launch geometry a halo one column short on either
    side (seam_cases.windowed_forward(short=...)), each move the reference by >= 100 x the bar
    the GPU test asserts for every precision (TapCase.rtol: the stage bars; the 16-conv list
    holds bf16x3 to f16x3's, as bf16w is everywhere)."""
    case = T.BY_NAME[name]
    blk = case.blk
    cap = S.block_max_length(pkg, blk)
    ws = S.block_windows(pkg, blk)
    worst = None

    def note(what, moved, ref):
        nonlocal worst
        r = _ratios(moved, ref, case.rtol)
        if worst is None or r[S.WIDEST] < worst[1][S.WIDEST]:
            worst = (what, r, moved)
        assert min(r.values()) >= MIN_RATIO, (name, what, moved, r)

    L = min(cap, max(S.mutant_length(w, cap) for w in ws))
    x, ref = T.tap_ref(pkg, name, L)
    got, _ = T.forward64(name, x, moved=T.widest_conv(blk))
    note("outer tap at d - 1", float(np.abs(got - ref).max()), ref)
    for w in ws:
        if not w.windowed:
            continue
        L = S.mutant_length(w, cap)
        x, ref = T.tap_ref(pkg, name, L)
        muts = S.mutants(blk, w, x, T.tap_state(name))
        assert np.abs(muts["exact"][0] - ref).max() == 0, (name, w.tag)
        for m in ("a:left", "a:right"):
            out, allowed = muts[m]
            d = np.abs(out - ref)
            assert not (d.max(axis=(0, 1)) > 0)[~allowed].any(), (name, w.tag, m)
            note(f"{w.tag} {m}", float(d.max()), ref)
    evidence(f"smallest mutant move / bar: {worst[0]} moved {worst[2]:.3g}: " +
             ", ".join(f"{p} {r:.3g}" for p, r in worst[1].items()))


# ----------------------------------------------------------------------------------------
# 4. upsampler cases
# ----------------------------------------------------------------------------------------
UPS = [c.name for c in T.UPS_CASES]


@pytest.mark.parametrize("name", UPS)
def test_ups_case_sits_where_it_says(pkg, name, evidence):
    case = T.UPS_BY_NAME[name]
    move = f"{name} no longer runs where it says ({case.why}): move the case"
    sig = {p: T.ups_signature(T.ups_host_plan(pkg, name, p)) for p in S.PRECISIONS}
    assert sig["f16x3"] == case.pin16 and sig["fp32"] == case.pin32, (move, sig)
    assert sig["bf16x3"] == sig["bf16w"] == sig["f16x3"]
    u, k = case.u, case.k
    rows = case.c0 // 2 * u
    assert k >= u and rows >= 32, "the split-precision kernels need 32 GEMM rows"
    what, rel, const = case.limit
    assert REL[rel](case.KT, T.UPS_LIMITS[const])
    # the split kernel runs the stage iff its taps per phase fit the runtime-KT instance
    assert case.pin16[0] == int(case.KT <= T.UPS_LIMITS[const]), move
    # the output-frame kernel is packed for k = 2u at the rates whose classes store whole runs
    frames_ok = k == 2 * u and (u in (2, 4) or u % 8 == 0) and case.c0 % 16 == 0 and \
        (rows // 2) % 32 == 0
    assert case.frames == frames_ok, move
    tiles, edges = T.ups_tiles(pkg, name), T.ups_edges(pkg, name)
    for tag, nt in tiles.items():   # every tile of the plan has its edge among the lengths
        on = [L for L in range(1, T.UPS_MAX_FRAMES + 1)
              if (L if tag == "frames" else case.columns(L)) == nt]
        assert on and set(on) <= set(edges), (move, tag, nt)
    Ls = T.ups_lengths(pkg, name)
    paths = set().union(*(case.store_paths(L) for L in Ls))
    assert paths == ({"float4", "masked float4"} if case.store == "float4" else {"scalar"}), paths
    assert case.store_paths(1) == ({"masked float4"} if case.store == "float4" else {"scalar"})
    assert Ls[:5] == [1, 2, 3, 4, 5] and max(Ls) <= T.UPS_MAX_FRAMES
    for e in edges:   # one column short of, on and past each edge
        assert {e - 1, e, e + 1} <= set(Ls)
    for T_, lens in T.ups_ragged_batches(pkg, name):
        assert T_ % 4 == 0 and T_ == max(lens) <= T.UPS_MAX_FRAMES
    odd = (k - u) % 2
    assert case.out_len(7) == 7 * u + odd, "k - u odd: L_out = u L + 1"
    evidence(f"KT {case.KT} {rel} {T.UPS_LIMITS[const]}, p {case.p}, rows {rows}, {case.store} stores, "
             f"row -> phase by {'shift' if u & (u - 1) == 0 else 'division'}, plan {case.pin16}, "
             f"tiles {tiles}, lengths {Ls}")


def test_ups_cases_cover_every_path():
    cs = T.UPS_CASES
    assert {c.store for c in cs if c.pin16[0]} == {"float4", "scalar"}
    assert {c.KT for c in cs} >= {1, 2, 3, 16, 17}
    assert {c.pin16[4][0] for c in cs} == {-1, 0, 1}, "both output-frame configurations"
    assert {c.u for c in cs} >= {1, 2, 3, 4, 5, 8, 16}
    assert {c.p for c in cs if (c.k - c.u) % 2} >= {0, 1, 2}
    assert any(c.signed for c in cs) and any(not c.pin16[0] for c in cs)


@pytest.mark.parametrize("name", UPS)
def test_ups_probe_values_are_exact(pkg, name, evidence):
    """ups.0 and the MRF behind it hold integers < 2^16 (the signed case: multiples of 0.1 in
    float64, under the same bound); the weights are small integers, every tap of every output
    channel distinct."""
    case = T.UPS_BY_NAME[name]
    w = T.ups_state(name)["ups.0.weight"]
    assert case.u % 7, "taps j and j + u of one phase have different weights"
    for co in range(case.c0 // 2):   # no (input channel, weight) pair twice in one output channel
        ci, j = np.nonzero(w[:, co, :])
        assert len(j) == case.k and len({(c, w[c, co, t]) for c, t in zip(ci, j)}) == case.k, co
    for j in range(case.k):
        assert set(np.unique(w[:, :, j])) == {0.0, 1.0 + j % 7} and (w[:, :, j] != 0).sum() == case.c0 // 2
    for key, v in T.ups_state(name).items():   # bf16w computes the same model
        t = torch.from_numpy(np.array(v))
        assert torch.equal(t.to(torch.bfloat16).float(), t), key
    top = 0.0
    Ls = T.ups_lengths(pkg, name)
    for L in Ls:
        r = T.ups_refs(name, L)
        assert np.array_equal(r["conv_pre"], np.asarray(T.ups_mel(name, L), np.float64))
        for tap in ("ups.0",) if case.signed else ("ups.0", "mrfs.0"):
            t = r[tap] * (10.0 if case.signed else 1.0)
            assert np.abs(t - np.round(t)).max() < 1e-6 and (case.signed or t.min() >= 0), tap
            top = max(top, float(np.abs(r[tap]).max()))
        assert r["ups.0"].shape[-1] == case.out_len(L) and np.abs(r["wav"]).max() < 0.8
    assert 0 < top < 2 ** 16
    evidence(f"largest activation {top:.0f}")


@pytest.mark.parametrize("name", UPS)
def test_probes_resolve_ups_mutants(pkg, name, evidence):
    """A dropped last tap, tap 0 stored in the neighbouring phase, a polyphase launch one
    column short and a padding off by one each move the float64 ups.0 tensor by >= 100 x the
    stage bar of every precision, at short lengths, an edge length and the longest (the
    padding crops the last tap off the first p / u frames: nothing to resolve below that)."""
    case = T.UPS_BY_NAME[name]
    Ls = T.ups_lengths(pkg, name)
    worst = None
    for L in (2 + case.p // case.u, 5 + case.p // case.u, Ls[-2], Ls[-1]):
        ref, muts = T.ups_mutants(name, L)
        assert np.array_equal(ref, T.ups_refs(name, L)["ups.0"])
        for m, out in muts.items():
            if m == "p off by one" and ref.shape[-1] == 1:
                continue
            moved = float(np.abs(out - ref).max())
            r = _ratios(moved, ref)
            if worst is None or r[S.WIDEST] < worst[1][S.WIDEST]:
                worst = (f"{m} at L {L}", r, moved)
            assert min(r.values()) >= MIN_RATIO, (name, m, L, moved, r)
    evidence(f"smallest mutant move / bar: {worst[0]} moved {worst[2]:.3g}: " +
             ", ".join(f"{p} {r:.3g}" for p, r in worst[1].items()))


def test_config_sweep_refusals_are_the_host_plans(pkg):
    """test_gpu_config_sweep.py counts a refusal at creation only where the host plan refuses
    the same configuration; the host refuses exactly HOST_REFUSED of its N_CFG x 4 pairs."""
    import test_gpu_config_sweep as W
    refused = [(seed, p) for seed in range(W.N_CFG) for p in W.PRECISIONS
               if W.host_refusal(pkg, W._draw(seed)[0], p) is not None]
    assert len(refused) == W.HOST_REFUSED, refused
    assert W.N_CFG * len(W.PRECISIONS) == 128
