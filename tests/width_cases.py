"""Configurations, coverage targets, references and bars of the channel-width tests
(test_widths_host.py, test_gpu_widths.py).  Not a test module and not a conftest: plain helpers.

What is under test: the code the kernels carry for channel widths off the power-of-two grid,
which no preset and no earlier fixture reaches —

* a partial last 16-channel group of the split-precision layer conv (conv_bf16x3.hip load_x /
  store_x, the `!full` branch: C_in = 13, 40, 50, 72, 100, 200), conv_pre on the caller's mel in
  both layouts included;
* GEMM row counts that are no multiple of the 32-row MFMA block or leave the last m-tile part
  full (M = 40, 50, 100, 160, 200, 250, 300, 320, 400; the epilogue masks of epilogue.h and the
  upsampler scatter);
* tile 3 as an LDS-ring layer conv (C = 200, or conv_pre with n_mels = 72 / 100), several
  m-tiles of the output-frame upsampler in both configurations, chunk tails and row tails of
  the fp32 kernel, stages of 17-31 channels (fp32 kernels inside a split-precision handle),
  conv_post / absmax / mrf_combine at odd channel counts.

TARGETS states, per configuration, which of these it exists for, as predicates on the plan
dump (hfg_debug_plan): a planner change that moves a configuration off its path fails the host
test instead of quietly testing something else.

No tolerance is introduced here: the stage bars are test_gpu_stages.py's (STAGE_RTOL and
stage_bar), the wav bar the project's 1e-4.
"""
import functools
import re
from dataclasses import dataclass
from typing import Dict, Tuple

import numpy as np
import torch

from oracle import config as C
from oracle import hifigan_np64 as N
from oracle import hifigan_torch as H
from oracle import prng
from test_gpu_stages import STAGE_RTOL, stage_bar  # noqa: F401  (the only stage tolerances used)

ATOL = 1e-4   # the project's wav bar
PRECISIONS = ("fp32", "bf16x3", "f16x3", "bf16w")
STAGE_PRECISIONS = ("fp32", "f16x3", "bf16x3")
RES_KERNELS = [3, 7, 11]
RES_DILATIONS = [[1, 3], [1, 5], [2, 4]]


def _cfg(n_mels, c0, rates, kernels):
    return C.GenConfig(n_mels=n_mels, upsample_rates=rates, upsample_kernel_sizes=kernels,
                       upsample_initial_channel=c0, resblock_kernel_sizes=list(RES_KERNELS),
                       resblock_dilation_sizes=[list(d) for d in RES_DILATIONS])


#                      n_mels  c0   rates          kernels            stage widths
CONFIGS = {
    "W96": _cfg(80, 96, [8, 4, 2], [16, 8, 4]),                 # 48, 24, 12
    "W320": _cfg(100, 320, [8, 8, 2, 2], [16, 16, 4, 4]),       # 160, 80, 40, 20
    "W400": _cfg(128, 400, [4, 4, 2], [8, 8, 4]),               # 200, 100, 50
    "ODD100": _cfg(13, 100, [2, 2, 2], [4, 4, 4]),              # 50, 25, 12
    "W160": _cfg(72, 160, [2, 8], [4, 16]),                     # 80, 40
    "W200R": _cfg(80, 200, [3, 5], [7, 11]),                    # 100, 50; L = 15 T
}
# standalone MRF / ResBlock entry (hfg_mrf_create)
MRF_WIDTHS = (20, 24, 25, 40, 48, 50, 80, 100, 160, 200)
MRF_DILATIONS = ((1, 3),) * 3
MRF_LENGTHS = (259, 512)
# the draw of the width sweep
SWEEP_C0 = (24, 40, 48, 80, 96, 100, 144, 160, 200, 320, 400)
SWEEP_MELS = (13, 40, 72, 80, 100, 128)
SWEEP_SEEDS = 16


# ----------------------------------------------------------------------------------------
# coverage targets: predicates on the plan dump
# ----------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Target:
    config: str
    precision: str
    layers: str                 # regular expression, full match on the layer's module name
    want: Tuple[Tuple[str, object], ...]   # (field of the plan's layer entry, value)
    why: str

    def matches(self, plan):
        """The layers of `plan` the pattern names (at least one), each checked by holds()."""
        return [L for L in plan["layers"] if re.fullmatch(self.layers, L["mod"])]

    def holds(self, layer):
        return all(layer_field(layer, k) == v for k, v in self.want)


def layer_field(layer, key):
    """A field of a plan layer entry; "frames" = (configuration, m-tiles) of the output-frame
    upsampler packing, "small" = (tile, m-tiles, chunks) of the small-tile packing."""
    if key == "frames":
        return tuple(layer["frames"][:2])
    if key == "small":
        return tuple(layer["small"][:3])
    return layer[key]


def _t(config, precision, layers, why, **want):
    return Target(config, precision, layers, tuple(sorted(want.items())), why)


K3, K7, K11 = r"\.resblocks\.0\.convs[12]\.\d", r"\.resblocks\.1\.convs[12]\.\d", \
    r"\.resblocks\.2\.convs[12]\.\d"
ANYK = r"\.resblocks\.\d\.convs[12]\.\d"
TARGETS = [
    # ---- W96: output-frame upsampler on 3 m-tiles; C = 48 rows 32..47 of a second m-tile;
    # C = 24 / 12: the fp32 kernels inside a split-precision handle, chunk tails
    _t("W96", "f16x3", "conv_pre", "96 rows on the 64-row tile: last m-tile half full",
       prec=1, tile=1, m_tiles=2, n_chunks=20),
    _t("W96", "f16x3", r"ups\.0", "frames cfg 0 with 3 m-tiles (rows_f = 192)", prec=1,
       frames=(0, 3)),
    _t("W96", "f16x3", "mrfs.0" + ANYK, "C = 48: tile 2, 2 m-tiles, 3 whole groups", prec=1,
       tile=2, m_tiles=2),
    _t("W96", "f16x3", "mrfs.1" + K3, "C = 24: fp32 kernel, CK 8 -> 3 chunks", prec=0, CK=8,
       n_chunks=3),
    _t("W96", "f16x3", "mrfs.1" + K7, "C = 24: fp32 kernel, CK 4 -> 6 chunks", prec=0, CK=4,
       n_chunks=6),
    _t("W96", "f16x3", "mrfs.2" + ANYK, "C = 12: fp32 kernel, 12 of 32 rows", prec=0, tile=2,
       m_tiles=1),
    _t("W96", "fp32", "conv_pre", "96 rows on the M64 tile: 2 m-tiles", prec=0, tile=1, m_tiles=2),
    # ---- W320: conv_pre reads a 100-channel mel on tile 3 (3 m-tiles, partial group of 4);
    # C = 160 AREG with a part-full second m-tile; frames cfg 0 with 10 / 5 m-tiles
    _t("W320", "f16x3", "conv_pre", "n_mels = 100 on tile 3 (LDS ring), 3 m-tiles, 7 groups",
       prec=1, tile=3, m_tiles=3, n_chunks=28),
    _t("W320", "f16x3", r"ups\.0", "frames cfg 0 with 10 m-tiles", prec=1, frames=(0, 10)),
    _t("W320", "f16x3", r"ups\.1", "frames cfg 0 with 5 m-tiles", prec=1, frames=(0, 5)),
    _t("W320", "f16x3", "mrfs.0" + ANYK, "C = 160: AREG tile, second m-tile 32 rows of 128",
       prec=1, tile=5, m_tiles=2),
    _t("W320", "f16x3", "mrfs.1" + ANYK, "C = 80: tile 1, second m-tile 16 rows", prec=1, tile=1,
       m_tiles=2),
    _t("W320", "f16x3", "mrfs.2" + ANYK, "C = 40: tile 2, partial group of 8, 8-row tail",
       prec=1, tile=2, m_tiles=2),
    _t("W320", "f16x3", "mrfs.3" + K7, "C = 20: fp32 kernel, CK 4 -> 5 chunks", prec=0, CK=4,
       n_chunks=5),
    _t("W320", "fp32", "conv_pre", "M128 tile, 3 m-tiles, C_in = 100 at CK 4", prec=0, tile=0,
       m_tiles=3, n_chunks=25),
    _t("W320", "fp32", r"ups\.0", "M128 tile, 10 m-tiles", prec=0, tile=0, m_tiles=10),
    # ---- W400: C = 200 on plain tile 3, 13 groups (the 13th half full)
    _t("W400", "f16x3", "mrfs.0" + K3, "C = 200: tile 3 (not AREG), 2 m-tiles, 13 groups x 2",
       prec=1, tile=3, m_tiles=2, n_chunks=26),
    _t("W400", "f16x3", "mrfs.0" + K11, "C = 200, k = 11 on tile 3: 13 groups x 6", prec=1,
       tile=3, m_tiles=2, n_chunks=78),
    _t("W400", "f16x3", "mrfs.1" + ANYK, "C = 100: tile 1, 7 groups (the 7th 4 channels)", prec=1,
       tile=1, m_tiles=2),
    _t("W400", "f16x3", "mrfs.2" + ANYK, "C = 50: tile 2, 4 groups (the 4th 2 channels)", prec=1,
       tile=2, m_tiles=2),
    _t("W400", "f16x3", r"ups\.0", "polyphase rows M = 800: 7 m-tiles, the 7th 32 rows", prec=1,
       tile=3, m_tiles=7, n_chunks=25),
    _t("W400", "fp32", r"ups\.0", "M128 tile, 7 m-tiles", prec=0, tile=0, m_tiles=7),
    _t("W400", "fp32", "mrfs.1" + K3, "C_in = 100 at CK 8: 13 chunks, the 13th half", prec=0,
       tile=1, CK=8, n_chunks=13),
    # ---- ODD100: every width off the grid; n_mels = 13 (one partial group and nothing else)
    _t("ODD100", "f16x3", "conv_pre", "C_in = 13: one partial group; 100 rows on tile 1", prec=1,
       tile=1, m_tiles=2, n_chunks=4),
    _t("ODD100", "f16x3", "mrfs.0" + ANYK, "C = 50 on tile 2", prec=1, tile=2, m_tiles=2),
    _t("ODD100", "f16x3", "mrfs.1" + K3, "C = 25 (odd rows): fp32 kernel, CK 8 -> 4 chunks",
       prec=0, CK=8, n_chunks=4),
    _t("ODD100", "f16x3", "mrfs.1" + K7, "C = 25: fp32 kernel, CK 4 -> 7 chunks", prec=0, CK=4,
       n_chunks=7),
    _t("ODD100", "f16x3", r"ups\.2", "25 -> 12 channels: fp32 upsampler, 24 rows", prec=0,
       tile=2, m_tiles=1),
    _t("ODD100", "fp32", "conv_pre", "C_in = 13 at CK 4: 4 chunks, the 4th one channel", prec=0,
       CK=4, n_chunks=4),
    _t("ODD100", "fp32", "mrfs.2" + K3, "C_in = 12 at CK 8: 2 chunks", prec=0, CK=8, n_chunks=2),
    # ---- W160: conv_pre (72 -> 160) on tile 3; frames cfg 1 with 5 m-tiles
    _t("W160", "f16x3", "conv_pre", "n_mels = 72 on tile 3: 5 groups (the 5th half), 2 m-tiles",
       prec=1, tile=3, m_tiles=2, n_chunks=20),
    _t("W160", "f16x3", r"ups\.1", "frames cfg 1 with 5 m-tiles (rows_f = 160)", prec=1,
       frames=(1, 5)),
    _t("W160", "f16x3", "mrfs.1" + ANYK, "C = 40 on tile 2", prec=1, tile=2, m_tiles=2),
    _t("W160", "fp32", "conv_pre", "C_in = 72 at CK 4 on the M128 tile, 2 m-tiles", prec=0,
       tile=0, m_tiles=2, n_chunks=18),
    # ---- W200R: odd rates (polyphase rows 300 / 250), conv_post at C = 50 and L % 4 != 0
    _t("W200R", "f16x3", r"ups\.0", "k = 7, u = 3: polyphase, M = 300 -> 3 m-tiles", prec=1,
       tile=3, m_tiles=3, frames=(-1, 0)),
    _t("W200R", "f16x3", r"ups\.1", "k = 11, u = 5: polyphase, M = 250, C_in = 100", prec=1,
       tile=3, m_tiles=2, n_chunks=14),
    _t("W200R", "fp32", r"ups\.1", "M128 tile, C_in = 100 at CK 8: 13 chunks", prec=0, tile=0,
       CK=8, n_chunks=13),
]


def targets(config, precision):
    return [t for t in TARGETS if t.config == config and t.precision == precision]


# ----------------------------------------------------------------------------------------
# kernel-instance names (hfg_profile_summary)
# ----------------------------------------------------------------------------------------
# conv1d_bf16x3<kt, TPC, WAVES_M, WAVES_N, WM, WN, WD, ups, np, AREG, fmt>; the geometry of a
# tile as the name prints it, from csrc/kernels.h kBf16x3Tiles
BF16X3_TILES = {1: (2, 1, 4, 2, 2, 2, False), 2: (4, 1, 4, 1, 2, 2, False),
                3: (2, 2, 2, 2, 4, 2, False), 4: (4, 2, 1, 1, 2, 2, False),
                5: (2, 2, 2, 2, 4, 2, True), 6: (2, 4, 1, 2, 4, 2, True)}


def bf16x3_instances(names):
    """{(kt, tile, ups)} of the conv1d_bf16x3 instances in a profile summary."""
    out = set()
    for n in names:
        m = re.fullmatch(r"conv1d_bf16x3<(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\w+), "
                         r"\d+, (\w+), \d+>", n)
        if m:
            geo = tuple(int(v) for v in m.groups()[1:7]) + (m.group(9) == "true",)
            tile = next(t for t, g in BF16X3_TILES.items() if g == geo)
            out.add((int(m.group(1)), tile, m.group(8) == "true"))
    return out


def fp32_instances(names):
    """{(kt, tile, CK, ups)} of the conv1d_mfma_f32<kt, WM, WN, WAVES_M, WAVES_N, CK, ups>
    instances in a profile summary (tile: 0 = M128, 1 = M64, 2 = M32)."""
    tiles = {(2, 2, 2, 2): 0, (2, 2, 1, 4): 1, (1, 4, 1, 4): 2}
    out = set()
    for n in names:
        m = re.fullmatch(r"conv1d_mfma_f32<(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\w+)>", n)
        if m:
            out.add((int(m.group(1)), tiles[tuple(int(v) for v in m.groups()[1:5])],
                     int(m.group(6)), m.group(7) == "true"))
    return out


def ups_frames_launches(summary):
    """{configuration: launches} of ups_bf16x3<WAVES_M, WAVES_N, WM, WN, np, fmt>."""
    out = {}
    for n, v in summary.items():
        m = re.fullmatch(r"ups_bf16x3<(\d+), (\d+), (\d+), (\d+), \d+, \d+>", n)
        if m:
            cfg = {(2, 2, 1, 4): 0, (1, 4, 1, 2): 1}[tuple(int(x) for x in m.groups())]
            out[cfg] = out.get(cfg, 0) + v["launches"]
    return out


def gen_taps(cfg):
    """{module: (GEMM taps, is an upsampler)} of a Generator's layers."""
    from test_capi_host import config_layers
    return {m: (-(-k // u), kind == 1) for m, kind, _, _, k, _, u in config_layers(cfg)}


def mrf_taps(kernels=tuple(RES_KERNELS), dilations=MRF_DILATIONS):
    """The same of a standalone MRF handle (hfg_mrf_create)."""
    return {f"resblocks.{j}.convs{c}.{m}": (k, False)
            for j, (k, dl) in enumerate(zip(kernels, dilations)) for c in (1, 2)
            for m in range(len(dl))}


def expected_instances(plan, taps, small):
    """({(kt, tile, ups)} of conv1d_bf16x3, {(kt, tile, CK, ups)} of conv1d_mfma_f32) that the
    layer launches of a handle with this plan run when every split-precision layer with a
    small-tile packing is forced onto it (small = 1) or off it (small = 0), upsamplers on the
    polyphase kernel.  taps: gen_taps / mrf_taps.  The instance's tap count is the layer's
    where the kernel has a compile-time instance for it (csrc/conv_bf16x3.hip g_entries3,
    kernels.h kt_specialised), else 0."""
    split, fp32 = set(), set()
    for L in plan["layers"]:
        if L["mod"] not in taps:
            continue
        kt, ups = taps[L["mod"]]
        if L["prec"] == 1:
            tile = L["small"][0] if small and L["small"][0] >= 0 else L["tile"]
            split.add((kt if kt in ((2,) if ups else (3, 5, 7, 11)) else 0, tile, ups))
        else:
            fp32.add((kt if kt in (2, 3, 5, 7, 11) else 0, L["tile"], L["CK"], ups))
    return split, fp32


# ----------------------------------------------------------------------------------------
# weights, handles, inputs, references
# ----------------------------------------------------------------------------------------
SEED = 171


@functools.lru_cache(maxsize=None)
def state(name):
    """Default-init-bounded PRNG weights of a configuration (shared: never modified)."""
    sd = C.make_state_dict(CONFIGS[name], seed=SEED)
    for v in sd.values():
        v.setflags(write=False)
    return sd


def _writable(sd):
    return {k: np.array(v) for k, v in sd.items()}


def bf16_rounded(sd):
    """The model bf16w computes: every conv weight rounded to bf16, biases fp32."""
    return {k: (torch.from_numpy(np.array(v)).to(torch.bfloat16).float().numpy()
                if k.endswith(".weight") else v) for k, v in sd.items()}


def host_handle(pkg, name, precision):
    """A host-only handle of the configuration with its weights committed."""
    h = pkg.Handle(pkg.make_config(**CONFIGS[name].kwargs(), precision=precision), -1)
    for k, v in state(name).items():
        h.set_weight(k, torch.from_numpy(np.array(v)))
    h.commit()
    return h


def make_generator(pkg, name, precision, dev):
    gen = pkg.HiFiGANGenerator(**CONFIGS[name].kwargs(), precision=precision).eval()
    gen.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state(name).items()})
    return gen.to(dev)


# frames per item: even, so W200R's L = 15 T has L % 4 != 0 only where a test asks (T = 33)
STAGE_B, STAGE_T = 2, 40


@functools.lru_cache(maxsize=None)
def mel(name, B=STAGE_B, T=STAGE_T):
    m = prng.mel_input(SEED + T, (B, CONFIGS[name].n_mels, T))
    m.setflags(write=False)
    return m


def _taps64(cfg, sd, m):
    taps = {}
    taps["wav"] = N.generator_forward(sd, cfg, m, tap=lambda n, t: taps.__setitem__(n, t.copy()))
    return taps


@functools.lru_cache(maxsize=None)
def refs(name, B=STAGE_B, T=STAGE_T):
    """({tap: float64 reference}, {tap: fp32 oracle}) of mel(name, B, T), "wav" included;
    computed once per session and shared."""
    cfg, sd, m = CONFIGS[name], state(name), mel(name, B, T)
    r32 = {}
    r32["wav"] = H.generator_forward(H.to_torch_state(_writable(sd)), cfg, torch.from_numpy(np.array(m)),
                                     tap=lambda n, t: r32.__setitem__(n, t.numpy().copy())).numpy()
    return _taps64(cfg, sd, m), r32


@functools.lru_cache(maxsize=None)
def refs_bf16w(name, B=STAGE_B, T=STAGE_T):
    """{tap: fp32 oracle on bf16-rounded weights} of mel(name, B, T), "wav" included: the model
    bf16w computes."""
    r = {}
    r["wav"] = H.generator_forward(H.to_torch_state(bf16_rounded(state(name))), CONFIGS[name],
                                   torch.from_numpy(np.array(mel(name, B, T))),
                                   tap=lambda n, t: r.__setitem__(n, t.numpy().copy())).numpy()
    return r


@functools.lru_cache(maxsize=None)
def wav_ref(name, B, T, bf16_weights=False, n=None, b=None):
    """The fp32 oracle's wav of mel(name, B, T) (bf16_weights: on bf16-rounded weights); with
    b / n: of item b alone on its first n frames."""
    sd = bf16_rounded(state(name)) if bf16_weights else state(name)
    m = np.array(mel(name, B, T))
    if b is not None:
        m = m[b:b + 1, :, :n]
    return H.generator_forward(H.to_torch_state(_writable(sd)), CONFIGS[name],
                               torch.from_numpy(m)).numpy()


def stage_names(name):
    out = ["conv_pre"]
    for i in range(len(CONFIGS[name].upsample_rates)):
        out += [f"ups.{i}", f"mrfs.{i}"]
    return out


def stage_bars(name, precision, B=STAGE_B, T=STAGE_T):
    """{stage: (bar, cond, scale)} by test_gpu_stages.stage_bar, cond = max|fp32 oracle -
    float64 reference| of the stage, scale = max|fp32 oracle|."""
    r64, r32 = refs(name, B, T)
    out = {}
    for s in stage_names(name):
        cond = float(np.abs(r32[s].astype(np.float64) - r64[s]).max())
        scale = float(np.abs(r32[s]).max())
        out[s] = (stage_bar(precision, scale, cond), cond, scale)
    return out


# ----------------------------------------------------------------------------------------
# tail sensitivity of the bars (float64 oracle alone; project code is never made wrong)
# ----------------------------------------------------------------------------------------
def stage_convs(name):
    """{stage: module of one conv feeding it}: conv_pre, the upsampler, and per MRF the conv in
    the middle of the last ResBlock's chain (convs2.0 of the k = 11 block: the most chunks; a
    wrong input channel passes through that conv alone, a wrong output row through a whole
    further dilation pair).

    How far one channel of one conv moves a stage depends on how active that channel happens
    to be.  Measured on the float64 oracle over all 12 convs of W400 mrfs.2, W320 mrfs.3,
    W96 mrfs.1 and W200R mrfs.1: 6.7 x to 1070 x the bf16x3 bar; convs reading a nearly
    silent channel (W400 mrfs.2 resblocks.0.convs2.0: 6.7 x) or sitting in W320's quiet
    20-channel stage (its convs1.0: 8.5 x - 9.4 x) stay under 10 x that bar while still 67 x
    or more over the f16x3 bar, a tenth of it."""
    out = {"conv_pre": "conv_pre"}
    for i in range(len(CONFIGS[name].upsample_rates)):
        out[f"ups.{i}"] = f"ups.{i}"
        out[f"mrfs.{i}"] = f"mrfs.{i}.resblocks.{len(RES_KERNELS) - 1}.convs2.0"
    return out


def tail_mutants(name) -> Dict[Tuple[str, str], dict]:
    """{(stage, "in" | "out"): float64 state dict with the last input channel ("in") or the
    last output row ("out": weights and bias) of that stage's conv zeroed}."""
    out = {}
    for stage, mod in stage_convs(name).items():
        transposed = mod.startswith("ups.")   # ConvTranspose1d weight: [C_in, C_out, k]
        for which in ("in", "out"):
            sd = {k: np.array(v, np.float64) for k, v in state(name).items()}
            w = sd[mod + ".weight"]
            if (which == "in") != transposed:
                w[:, -1, :] = 0.0
            else:
                w[-1, :, :] = 0.0
            if which == "out":
                sd[mod + ".bias"][-1] = 0.0
            out[stage, which] = sd
    return out
