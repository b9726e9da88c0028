"""Generate tests/golden/plan_index.json: the plan fingerprint (``hfg_debug_plan``) and the
workspace sizes of a fixed list of host-only handles.

The fixture pins what the planner decides (tiles, packings, offsets, whole-ResBlock windows,
halos and splits, thin stages), every packed byte (sha256 of the packed image) and the
workspace arithmetic, so a change of the host orchestration that means to keep the schedule
can be checked on the CPU.  Regenerate it only with a change that means to move the plan,
from the library of the commit BEFORE that change where the change is a refactor:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_plan_index.py

``tests/test_plan_host.py`` imports ``cases`` / ``record`` from here and asserts equality.
"""
from __future__ import annotations

import functools
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import config as C, prng  # noqa: E402

OUT = os.path.join(HERE, "plan_index.json")
PRECISIONS = ("fp32", "bf16x3", "bf16w", "f16x3")
# the knobs the planner reads, each at its non-default value
PLAN_KNOBS = (("FUSED_RB", 0), ("RB_SPLIT", 0), ("FUSE_POST", 0), ("AREG_TALL", 0))
WS_B = (1, 2, 3, 16, 32)
WS_T = (1, 17, 32, 62, 2048, 8192)
MRF_L = (1, 255, 256, 4096)
# handles whose dump is stored verbatim (the others: its sha256)
VERBATIM = ("gen/v1/f16x3", "gen/v2star/bf16x3")
V1_KERNELS, V1_DILS = [3, 7, 11], [[1, 3, 5]] * 3
# channel widths off the power-of-two grid (tests/width_cases.py): every configuration in
# every precision, and the standalone MRF entry at four of its widths
WIDTH_MRF = (24, 40, 100, 200)


def _width_cases():
    tests = os.path.dirname(HERE)
    if tests not in sys.path:
        sys.path.insert(0, tests)
    import width_cases
    return width_cases


def cases():
    """[(name, kind, spec)]: kind "gen" spec (config name, precision, knob or None), kind
    "mrf" spec (channels, kernels, dilations, resblock, precision)."""
    out = []
    for preset in ("v1", "v2star", "nonexact"):
        for prec in PRECISIONS:
            out.append((f"gen/{preset}/{prec}", "gen", (preset, prec, None)))
    for prec in ("fp32", "f16x3"):
        out.append((f"gen/release_v3/{prec}", "gen", ("release_v3", prec, None)))
    for knob, v in PLAN_KNOBS:
        out.append((f"gen/v1/f16x3/{knob}={v}", "gen", ("v1", "f16x3", (knob, v))))
    for prec in ("f16x3", "bf16x3"):
        for rb in ("1", "2"):
            for ch in (8, 16, 32, 64, 128):
                out.append((f"mrf/C{ch}/rb{rb}/{prec}", "mrf", (ch, V1_KERNELS, V1_DILS, rb, prec)))
        # (k-1)/2 * d = 30 > rb_marg(128) = 28: k = 11 falls back to layer by layer
        out.append((f"mrf/C128/marg/{prec}", "mrf", (128, V1_KERNELS, [[1, 3, 6]] * 3, "1", prec)))
        # (k-1) * d = 130 > kBf16x3MaxHalo = 128: that layer runs the fp32 kernel
        out.append((f"mrf/C64/halo/{prec}", "mrf", (64, V1_KERNELS, [[1, 3, 13]] * 3, "1", prec)))
    W = _width_cases()
    for name in W.CONFIGS:
        for prec in PRECISIONS:
            out.append((f"gen/{name}/{prec}", "gen", (name, prec, None)))
    for ch in WIDTH_MRF:
        out.append((f"mrf/C{ch}/rb1/f16x3", "mrf",
                    (ch, V1_KERNELS, [list(d) for d in W.MRF_DILATIONS], "1", "f16x3")))
    return out


@functools.lru_cache(maxsize=None)
def _gen_state(name):
    """(config, seed-0 weights) of a generator, made once and shared (never modified)."""
    if name == "release_v3":
        from tts_sambert_hifigan_amd import synth as S
        return S.RELEASE_V3, S.random_state_dict(S.RELEASE_V3, seed=0)
    cfg = C.PRESETS[name] if name in C.PRESETS else _width_cases().CONFIGS[name]
    return cfg, C.make_state_dict(cfg, seed=0)


def _mrf_state_dict(ch, kernels, dils, resblock, seed=0):
    sd = {}
    for j, (k, dl) in enumerate(zip(kernels, dils)):
        for which in (("convs",) if resblock == "2" else ("convs1", "convs2")):
            for m in range(len(dl)):
                key = f"resblocks.{j}.{which}.{m}"
                bound = 1.0 / np.sqrt(ch * k)
                sd[key + ".weight"] = prng.uniform_sym(seed, key + ".weight", (ch, ch, k), bound)
                sd[key + ".bias"] = prng.uniform_sym(seed, key + ".bias", (ch,), bound)
    return sd


def record(pkg, kind, spec):
    """{"plan": the handle's hfg_debug_plan dict, + out_len / ws (gen) or ws (mrf)}."""
    pkg.schedule_clear()
    try:
        if kind == "gen":
            name, prec, knob = spec
            if knob:
                pkg.schedule_override(*knob)
            cfg, sd = _gen_state(name)
            h = pkg.Handle(pkg.make_config(**cfg.kwargs(), precision=prec), -1)
        else:
            ch, kernels, dils, rb, prec = spec
            sd = _mrf_state_dict(ch, kernels, dils, rb)
            h = pkg.Handle(pkg._lib.make_mrf_config(ch, kernels, dils, prec, resblock=rb), -1,
                           mrf=True)
    finally:
        pkg.schedule_clear()
    for k, v in sd.items():
        h.set_weight(k, torch.from_numpy(v))
    rec = {"plan": h.plan()}
    if kind == "gen":
        rec["out_len"] = [h.out_len(t) for t in WS_T]
        rec["ws"] = [[h.workspace_bytes(b, t) for t in WS_T] for b in WS_B]
    else:
        rec["ws"] = [[h.mrf_workspace_bytes(b, n) for n in MRF_L] for b in WS_B]
    return rec


def canonical_sha(plan) -> str:
    return hashlib.sha256(json.dumps(plan, sort_keys=True, separators=(",", ":")).encode()).hexdigest()


def stored(name, rec):
    """The fixture's form of one record: the dump verbatim or its sha256."""
    out = dict(rec)
    if name not in VERBATIM:
        out["plan"] = canonical_sha(out["plan"])
    return out


def main():
    import __graft_entry__ as ge
    pkg = ge.load_package()
    index = {name: stored(name, record(pkg, kind, spec)) for name, kind, spec in cases()}
    with open(OUT, "w") as f:
        json.dump(index, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print(f"{len(index)} handles -> {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
