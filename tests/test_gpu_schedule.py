"""Launch fingerprint of the forward schedule against tests/golden/schedule_index.json.

Per case the profile summary of one forward reduced to {kernel instance: [launches, flop,
bytes]} (no times).  The instance names carry the template arguments, so they pin from
outside what the host orchestration decides per call: tile picks, the frames / polyphase
upsampler, persistent grids, ResBlock splits, concurrent ResBlocks, the fused conv_post, the
two-stream batch split (a split forward's halves count as one launch with summed figures).
The fixture was recorded on an MI355X before the host orchestration was cut into plan / pack
/ forward units (tests/golden/make_schedule_index.py); the cases are the smallest shapes that
reach each branch."""
import functools
import json
import os

import pytest
import torch

from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu
INDEX_PATH = os.path.join(GOLDEN_DIR, "schedule_index.json")

KNOB_VARIANTS = ({}, {"FUSED_RB": 0}, {"RB_SPLIT": 0}, {"FUSE_POST": 0}, {"SMALL_TILE": 1},
                 {"SMALL_TILE": 0}, {"RB_CONC": 0}, {"RB_CONC": 1}, {"UPS_FRAMES": 2},
                 {"AREG_TALL": 0}, {"RB_PERSIST": 0})


def _case(model, precision, B, T, knobs=None, lengths=None, entry="forward"):
    return dict(model=model, precision=precision, B=B, T=T, knobs=knobs or {}, lengths=lengths,
                entry=entry)


def cases():
    """{case id: spec}; model "v1" / "v2star" / "nonexact" / "release_v3", or "mrf<C>" (V1's
    ResBlock lists at C channels on an MRF-only handle, T = its length L)."""
    out = {}
    for kn in KNOB_VARIANTS:
        tag = ",".join(f"{k}={v}" for k, v in kn.items()) or "default"
        out[f"v1-f16x3-1x32-{tag}"] = _case("v1", "f16x3", 1, 32, kn)
    out["v1-f16x3-2x17-ragged"] = _case("v1", "f16x3", 2, 17, lengths=[17, 5])
    out["v1-f16x3-1x2048"] = _case("v1", "f16x3", 1, 2048)
    out["v1-f16x3-2x2048"] = _case("v1", "f16x3", 2, 2048)
    for prec in ("fp32", "bf16x3", "bf16w"):
        out[f"v1-{prec}-2x64"] = _case("v1", prec, 2, 64)
    for prec in ("bf16x3", "fp32"):
        out[f"v2star-{prec}-2x64"] = _case("v2star", prec, 2, 64)
    out["nonexact-f16x3-2x33"] = _case("nonexact", "f16x3", 2, 33)
    out["release_v3-f16x3-2x64"] = _case("release_v3", "f16x3", 2, 64)
    for ch in (16, 64):
        out[f"mrf{ch}-f16x3-2x300-mrf"] = _case(f"mrf{ch}", "f16x3", 2, 300, entry="mrf")
        out[f"mrf{ch}-f16x3-2x300-resblock1"] = _case(f"mrf{ch}", "f16x3", 2, 300, entry="resblock1")
    return out


CASES = cases()


@functools.lru_cache(maxsize=None)
def _weights(model):
    """Seeded weights of one model, made once and shared (never modified)."""
    from oracle import config as C
    if model == "release_v3":
        from tts_sambert_hifigan_amd import synth as S
        return S.RELEASE_V3, S.random_state_dict(S.RELEASE_V3, seed=7)
    return C.PRESETS[model], C.make_state_dict(C.PRESETS[model], seed=7)


def run_case(pkg, spec, dev):
    """One profiled forward of `spec` on a fresh handle created under its knobs:
    ({label: [launches, flop, bytes]}, output tensor on the host)."""
    g = torch.Generator().manual_seed(1000 * spec["B"] + spec["T"])
    try:
        for k, v in spec["knobs"].items():
            pkg.schedule_override(k, v)
        if spec["model"].startswith("mrf"):
            ch = int(spec["model"][3:])
            mod = pkg.MRF(ch, precision=spec["precision"]).eval()
            with torch.no_grad():
                for p in mod.parameters():
                    p.copy_((torch.rand(p.shape, generator=g) - 0.5) * 0.1)
            mod = mod.to(dev)
            x = torch.randn(spec["B"], ch, spec["T"], generator=g).to(dev)
        else:
            cfg, sd = _weights(spec["model"])
            mod = pkg.HiFiGANGenerator(**cfg.kwargs(), precision=spec["precision"]).eval()
            mod.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
            mod = mod.to(dev)
            x = torch.randn(spec["B"], cfg.n_mels, spec["T"], generator=g).to(dev)
        h = mod._handle_for(dev)
    finally:
        pkg.schedule_clear()
    h.profile_reset()
    h.set_profiling(True)
    with torch.no_grad():
        if spec["entry"] == "mrf":
            y = mod(x)
        elif spec["entry"] == "resblock1":
            y = mod._run_block(x, mod.channels, 1)
        else:
            y = mod(x, lengths=spec["lengths"])
    torch.cuda.synchronize()
    h.set_profiling(False)
    prof = h.profile_summary()
    h.profile_reset()
    return {k: [v["launches"], v["flop"], v["bytes"]] for k, v in prof.items()}, y.cpu()


@pytest.fixture(scope="module")
def index():
    with open(INDEX_PATH) as f:
        return json.load(f)


def test_fixture_lists_every_case(index):
    assert sorted(index) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_launches_match_fixture(pkg, index, name):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    got, _ = run_case(pkg, CASES[name], torch.device("cuda:0"))
    want = index[name]
    assert sorted(got) == sorted(want), f"{name}: kernel instances differ"
    for label in want:
        assert got[label] == want[label], f"{name}: {label}: [launches, flop, bytes] differ"


def test_profile_summary_sizes_its_buffer(pkg):
    """hfg_profile_summary into a buffer of exactly the size its refusal names holds the
    whole JSON: the labels and launch counts of a 64 KiB buffer's."""
    import ctypes
    import re
    from oracle import config as C
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    dev = torch.device("cuda:0")
    cfg = C.GenConfig(n_mels=16, upsample_rates=[2, 2], upsample_kernel_sizes=[4, 4],
                      upsample_initial_channel=64, resblock_kernel_sizes=[3],
                      resblock_dilation_sizes=[[1, 3]])
    mod = pkg.HiFiGANGenerator(**cfg.kwargs(), precision="f16x3").eval()
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in C.make_state_dict(cfg, seed=7).items()})
    mod = mod.to(dev)
    h = mod._handle_for(dev)
    h.profile_reset()
    h.set_profiling(True)
    with torch.no_grad():
        mod(torch.randn(1, cfg.n_mels, 8, generator=torch.Generator().manual_seed(8)).to(dev))
    torch.cuda.synchronize()
    h.set_profiling(False)
    big = h.profile_summary()  # a 64 KiB buffer
    assert big and all(v["launches"] >= 1 for v in big.values())
    assert h.lib.hfg_profile_summary(h.ptr, ctypes.create_string_buffer(1), 1) == -22
    n = int(re.search(r"buffer too small \((\d+) needed\)",
                      h.lib.hfg_last_error().decode()).group(1))
    exact = ctypes.create_string_buffer(n)
    assert h.lib.hfg_profile_summary(h.ptr, exact, n) == 0
    got = json.loads(exact.value.decode())
    assert len(exact.value) == n - 1
    assert {k: v["launches"] for k, v in got.items()} == {k: v["launches"] for k, v in big.items()}
    assert h.lib.hfg_profile_summary(h.ptr, ctypes.create_string_buffer(n - 1), n - 1) == -22
    h.profile_reset()
