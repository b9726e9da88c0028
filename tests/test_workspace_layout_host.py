"""The forward workspace layout (csrc/handle.h ``WsLayout``, computed in plan.cpp, printed by
``hfg_debug_workspace``) on host-only handles: the layout the public sizes total and the launch
schedule takes every pointer from.  tests/golden/plan_index.json pins the totals
(tests/test_plan_host.py); this pins that the regions the schedule writes stay inside them:
for every handle of ``make_plan_index.cases()`` over that file's ``WS_B x WS_T`` grid (MRF
handles: ``WS_B x MRF_L``), with and without ``taps``,

* ``total`` equals ``workspace_bytes`` / ``mrf_workspace_bytes`` (taps: is at most that),
* parts are disjoint and inside ``total``; regions 256-byte aligned, disjoint, inside their part,
* every activation region holds 4 * B_part * max_i(C_i * L_i) bytes and the length table
  4 * (n_up + 1) * B_part, both computed here from the configuration,
* the slot region is non-empty exactly in f16x3 and bf16w,
* two parts exactly when B >= 2 and B * T >= 4096,
* the per-ResBlock triples are present exactly where some stage runs concurrent ResBlocks,
  recomputed here from the threshold and the stage shapes.
"""
import importlib.util
import os

import pytest
import torch

from conftest import GOLDEN_DIR

_spec = importlib.util.spec_from_file_location("make_plan_index",
                                               os.path.join(GOLDEN_DIR, "make_plan_index.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

CASES = M.cases()
SPLIT_MIN_FRAMES = 4096   # hfg_handle::kSplitMinFrames
CONC_BLOCKS = 2048        # hfg_handle::kConcBlocks
ACTIVATIONS = ("X", "R", "Tb", "MRF")


def _handle(pkg, kind, spec):
    """(handle with its weights set, description of what the layout depends on)."""
    pkg.schedule_clear()
    try:
        if kind == "gen":
            name, prec, knob = spec
            if knob:
                pkg.schedule_override(*knob)
            cfg, sd = M._gen_state(name)
            kw = cfg.kwargs()
            h = pkg.Handle(pkg.make_config(**kw, precision=prec), -1)
            c0 = kw["upsample_initial_channel"]
            ups = list(zip(kw["upsample_rates"], kw["upsample_kernel_sizes"]))
            desc = dict(prec=prec, c0=c0, ups=ups, n_res=len(kw["resblock_kernel_sizes"]),
                        chans=[c0 >> (i + 1) for i in range(len(ups))])
        else:
            ch, kernels, dils, rb, prec = spec
            sd = M._mrf_state_dict(ch, kernels, dils, rb)
            h = pkg.Handle(pkg._lib.make_mrf_config(ch, kernels, dils, prec, resblock=rb), -1,
                           mrf=True)
            desc = dict(prec=prec, ch=ch)
    finally:
        pkg.schedule_clear()
    for k, v in sd.items():
        h.set_weight(k, torch.from_numpy(v))
    return h, desc


def _stage_lengths(ups, T):
    """[T, L_1, ..]: L_out = (L_in - 1) u - 2 ((k - u) // 2) + k per stage."""
    L = [T]
    for u, k in ups:
        L.append((L[-1] - 1) * u - 2 * ((k - u) // 2) + k)
    return L


def _check_regions(lay, total_max):
    """Parts disjoint and inside total; regions aligned, disjoint, inside their part."""
    assert lay["total"] <= total_max
    end = 0
    for p in lay["parts"]:
        assert p["off"] >= end and p["off"] % 256 == 0, p
        end = p["off"] + p["bytes"]
        at = p["off"]
        for r in p["regions"]:
            assert r["off"] % 256 == 0 and r["bytes"] >= 0, r
            assert r["off"] >= at, (r, "overlaps the region before it")
            at = r["off"] + r["bytes"]
        assert at <= end, p
    assert end <= lay["total"]
    assert [p["b0"] for p in lay["parts"]] == [0, lay["parts"][0]["B"]][:len(lay["parts"])]


def _check_gen(h, d, thin, B, T, taps):
    lay = h.workspace_layout(B, T, taps=taps)
    ws = h.workspace_bytes(B, T)
    if not taps:
        assert lay["total"] == ws
    _check_regions(lay, ws)
    split = B >= 2 and B * T >= SPLIT_MIN_FRAMES
    assert len(lay["parts"]) == (2 if split and not taps else 1)
    assert sum(p["B"] for p in lay["parts"]) == B
    L = _stage_lengths(d["ups"], T)
    item = max([d["c0"] * T] + [c * max(l, 0) for c, l in zip(d["chans"], L[1:])])
    for p in lay["parts"]:
        Bp = p["B"]
        regions = {r["name"]: r for r in p["regions"]}
        assert len(regions) == len(p["regions"])
        # concurrent ResBlocks: only where the forward is one part on one stream, in a stage
        # that is not thin, of 2.. ResBlocks, whose convs leave tile-3 slots idle
        conc = not split and d["n_res"] >= 2 and any(
            not thin[i] and Bp * -(-L[i + 1] // 256) * -(-c // 128) < CONC_BLOCKS
            for i, c in enumerate(d["chans"]))
        triples = [f"rb{j}.{x}" for j in range(d["n_res"]) for x in ("R", "Tb", "out")]
        want = list(ACTIVATIONS) + (triples if conc else []) + ["table", "slots"]
        assert [r["name"] for r in p["regions"]] == want, (B, T, taps)
        for name in want[:-2]:
            assert regions[name]["bytes"] >= 4 * Bp * item, (name, B, T)
        assert regions["table"]["bytes"] >= 4 * (len(d["ups"]) + 1) * Bp
        assert (regions["slots"]["bytes"] > 0) == (d["prec"] in ("f16x3", "bf16w"))


def _check_mrf(h, d, B, L, taps):
    lay = h.workspace_layout(B, L, taps=taps)
    assert lay["total"] == h.mrf_workspace_bytes(B, L)
    _check_regions(lay, lay["total"])
    assert len(lay["parts"]) == 1 and lay["parts"][0]["B"] == B
    regions = {r["name"]: r for r in lay["parts"][0]["regions"]}
    assert list(regions) == ["R", "Tb", "slots"]
    for name in ("R", "Tb"):
        assert regions[name]["bytes"] >= 4 * B * d["ch"] * L
    assert (regions["slots"]["bytes"] > 0) == (d["prec"] in ("f16x3", "bf16w"))


@pytest.mark.parametrize("name,kind,spec", CASES, ids=[c[0] for c in CASES])
def test_workspace_layout(pkg, name, kind, spec):
    h, d = _handle(pkg, kind, spec)
    # which stages run the one-launch thin MRF is the plan's choice (tests/test_plan_host.py)
    thin = [bool(st["thin"]) for st in h.plan()["stages"]]
    for taps in (False, True):
        for B in M.WS_B:
            if kind == "gen":
                for T in M.WS_T:
                    _check_gen(h, d, thin, B, T, taps)
            else:
                for L in M.MRF_L:
                    _check_mrf(h, d, B, L, taps)


def test_workspace_layout_reports_errors(pkg):
    """A buffer that is too small and empty shapes are refused, as hfg_debug_plan does."""
    import ctypes
    from oracle import config as C
    h = pkg.Handle(pkg.make_config(**C.V2STAR.kwargs(), precision="f16x3"), -1)
    assert h.workspace_layout(3, 1366)["total"] == h.workspace_bytes(3, 1366)  # no weights needed
    small = ctypes.create_string_buffer(16)
    assert h.lib.hfg_debug_workspace(h.ptr, 1, 16, 0, small, len(small)) == -22
    big = ctypes.create_string_buffer(1 << 14)
    assert h.lib.hfg_debug_workspace(h.ptr, 0, 16, 0, big, len(big)) == -22
    assert h.lib.hfg_debug_workspace(h.ptr, 1, 0, 0, big, len(big)) == -22
    assert h.lib.hfg_debug_workspace(None, 1, 16, 0, big, len(big)) == -22
