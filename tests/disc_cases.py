"""Weights, inputs and lengths of the discriminator tests (host, GPU and the fixture maker).

Weights come from ``oracle/prng.py`` keyed by ``(seed, state-dict key)``: ``weight_v`` and
``bias`` at PyTorch's default bound ``1 / sqrt(fan_in)``, ``weight_g = gain_l * |v|`` (the norm
per output channel) with one gain per layer.  With the default init (gain 1) the maps decay
about 2x per layer and the last ones are mostly bias, so a wrong tap there would hide under any
bar; the gains below keep every map of the parity inputs at unit scale (the condition
``test_discriminators_host.py`` asserts on the float64 oracle: peak in [0.1, 4], standard
deviation at least 0.05 of the peak).  Weight shapes do not depend on the period, so one period
set and one scale set per seed serve every case; they are built once per process.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from oracle import prng

import discriminator_oracle as DO

SEED_PERIOD = 31
SEED_SCALE = 32
SEED_MSD = (32, 33, 34)      # MultiScaleDiscriminator.discriminators.{0, 1, 2}
SEED_MPD = (31, 35, 36, 37, 38)
WAV_SEED = 5
WAV_STD = 0.3

# one gain per layer (convs.0 .. conv_post)
PERIOD_GAINS = (1.0, 2.5, 2.5, 2.5, 2.5, 2.5)
SCALE_GAINS = (1.5, 2.5, 2.5, 2.5, 4.0, 6.0, 4.0, 4.0)
# the entry gain of MultiScaleDiscriminator.discriminators.{0, 1, 2}: each pooling of a white
# input halves its variance, so the pooled scales start higher to reach the same levels
MSD_ENTRY_GAINS = (1.5, 2.7, 3.6)

PERIODS = DO.PERIODS


def period_lengths(p: int):
    """T and what it exercises: H = 1 on every layer; a reflect pad of 1; no pad,
    H 243 -> 81 -> 27 -> 9 -> 3; pad p - 1, H 244 -> 82 -> 28 -> 10 -> 4."""
    return [p, 2 * p - 1, 243 * p, 243 * p + 1]


SCALE_LENGTHS = [1, 63, 64, 65, 257]
MSD_LENGTHS = [1, 257]


def _state(seed: int, layers, gains, conv2d: bool):
    sd = {}
    mods = [f"convs.{i}" for i in range(len(layers) - 1)] + ["conv_post"]
    for mod, (ci, co, k, _, _, g), gain in zip(mods, layers, gains):
        fan_in = (ci // g) * k
        bound = 1.0 / math.sqrt(fan_in)
        shape = (co, ci // g, k) + ((1,) if conv2d else ())
        v = prng.uniform_sym(seed, mod + ".weight_v", shape, bound)
        norm = np.sqrt((v.astype(np.float64).reshape(co, -1) ** 2).sum(axis=1))
        sd[mod + ".weight_g"] = torch.from_numpy(
            (gain * norm).astype(np.float32).reshape((co,) + (1,) * (len(shape) - 1)))
        sd[mod + ".weight_v"] = torch.from_numpy(v)
        sd[mod + ".bias"] = torch.from_numpy(prng.uniform_sym(seed, mod + ".bias", (co,), bound))
    return sd


@functools.lru_cache(maxsize=None)
def period_state(seed: int = SEED_PERIOD):
    """A PeriodDiscriminator state dict (8.2 M parameters), whatever the period."""
    return _state(seed, DO.PERIOD_LAYERS + [DO.PERIOD_POST], PERIOD_GAINS, True)


@functools.lru_cache(maxsize=None)
def scale_state(seed: int = SEED_SCALE, entry_gain: float = SCALE_GAINS[0]):
    """A ScaleDiscriminator state dict (9.9 M parameters)."""
    return _state(seed, DO.SCALE_LAYERS + [DO.SCALE_POST], (entry_gain,) + SCALE_GAINS[1:], False)


def msd_states():
    return [scale_state(s, g) for s, g in zip(SEED_MSD, MSD_ENTRY_GAINS)]


def msd_state_dict():
    """MultiScaleDiscriminator.state_dict() layout."""
    return {f"discriminators.{i}.{k}": v for i, sd in enumerate(msd_states())
            for k, v in sd.items()}


def wav(T: int, B: int = 1, seed: int = WAV_SEED) -> torch.Tensor:
    """[B, 1, T] float32, 0.3 * N(0, 1); item b of any batch is item b of a wider one."""
    rows = [prng.normal(seed + 1000 * b, "wav", (T,), WAV_STD) for b in range(B)]
    return torch.from_numpy(np.stack(rows)[:, None, :])


def loss_pair(T: int = 257):
    """The fixture pair of the loss values: real, fake = 0.9 real + 0.01 randn."""
    real = wav(T)
    noise = torch.from_numpy(prng.normal(WAV_SEED, "fake-noise", (1, 1, T)))
    return real, 0.9 * real + 0.01 * noise


def f64(sd):
    return {k: v.double() for k, v in sd.items()}
