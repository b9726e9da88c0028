"""The reference's discriminators (models/hifigan.py:286-616) and the loss formulas that read
them (models/losses.py:475-623) restated as plain ATen calls on CPU tensors, in the precision
of the tensors the caller passes (float32 or float64): the checker of the device
discriminators.  TEST INFRASTRUCTURE ONLY, in the pattern of ``oracle/hifigan_torch.py``.

A state dict is the reference module's own (``convs.N.weight_g`` / ``weight_v`` / ``bias``,
``conv_post.*``; or plain ``weight``), as torch tensors.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import torch
import torch.nn.functional as F

# (C_in, C_out, k, stride, pad, groups)
SCALE_LAYERS = [(1, 128, 15, 1, 7, 1), (128, 128, 41, 2, 20, 4), (128, 256, 41, 2, 20, 16),
                (256, 512, 41, 4, 20, 16), (512, 1024, 41, 4, 20, 16),
                (1024, 1024, 41, 1, 20, 16), (1024, 1024, 5, 1, 2, 1)]
SCALE_POST = (1024, 1, 3, 1, 1, 1)
PERIOD_LAYERS = [(1, 32, 5, 3, 2, 1), (32, 128, 5, 3, 2, 1), (128, 512, 5, 3, 2, 1),
                 (512, 1024, 5, 3, 2, 1), (1024, 1024, 5, 1, 2, 1)]
PERIOD_POST = (1024, 1, 3, 1, 1, 1)
PERIODS = (2, 3, 5, 7, 11)


def folded(sd: Dict[str, torch.Tensor], mod: str, dtype) -> Tuple[torch.Tensor, torch.Tensor]:
    """(weight, bias) of module ``mod`` in ``dtype``; weight norm folded in that precision as
    ``torch._weight_norm(v, g, 0)`` (what the reference's hook computes at forward time)."""
    if mod + ".weight_g" in sd:
        w = torch._weight_norm(sd[mod + ".weight_v"].to(dtype), sd[mod + ".weight_g"].to(dtype), 0)
    else:
        w = sd[mod + ".weight"].to(dtype)
    return w, sd[mod + ".bias"].to(dtype)


def scale_forward(sd, x: torch.Tensor) -> List[torch.Tensor]:
    """ScaleDiscriminator.forward: the 8 feature maps of x [B, 1, T] (the last is the output)."""
    maps = []
    for i, (_, _, _, s, p, g) in enumerate(SCALE_LAYERS):
        w, b = folded(sd, f"convs.{i}", x.dtype)
        x = F.leaky_relu(F.conv1d(x, w, b, stride=s, padding=p, groups=g), 0.1)
        maps.append(x)
    w, b = folded(sd, "conv_post", x.dtype)
    maps.append(F.conv1d(x, w, b, stride=1, padding=1))
    return maps


def pool(x: torch.Tensor, times: int) -> torch.Tensor:
    for _ in range(times):
        x = F.avg_pool1d(x, kernel_size=4, stride=2, padding=2)
    return x


def msd_forward(sds: Sequence[dict], x: torch.Tensor) -> List[List[torch.Tensor]]:
    """MultiScaleDiscriminator.forward: scale i sees x pooled i times."""
    return [scale_forward(sd, pool(x, i)) for i, sd in enumerate(sds)]


def period_forward(sd, x: torch.Tensor, period: int) -> List[torch.Tensor]:
    """PeriodDiscriminator.forward: the 6 feature maps of x [B, 1, T]."""
    B, C, T = x.shape
    if T % period:
        x = F.pad(x, (0, period - T % period), mode="reflect")
    x = x.view(B, C, x.shape[2] // period, period)
    maps = []
    for i, (_, _, _, s, p, _) in enumerate(PERIOD_LAYERS):
        w, b = folded(sd, f"convs.{i}", x.dtype)
        x = F.leaky_relu(F.conv2d(x, w, b, stride=(s, 1), padding=(p, 0)), 0.1)
        maps.append(x)
    w, b = folded(sd, "conv_post", x.dtype)
    maps.append(F.conv2d(x, w, b, stride=1, padding=(1, 0)))
    return maps


def mpd_forward(sds: Sequence[dict], x: torch.Tensor, periods=PERIODS) -> List[List[torch.Tensor]]:
    return [period_forward(sd, x, p) for sd, p in zip(sds, periods)]


def scale_shapes(T: int, pools: int) -> List[Tuple[int, int]]:
    L = T
    for _ in range(pools):
        L = L // 2 + 1
    out = []
    for (_, co, k, s, p, _) in SCALE_LAYERS + [SCALE_POST]:
        L = (L + 2 * p - k) // s + 1
        out.append((co, L))
    return out


def period_shapes(T: int, period: int) -> List[Tuple[int, int, int]]:
    H = -(-T // period)
    out = []
    for (_, co, k, s, p, _) in PERIOD_LAYERS + [PERIOD_POST]:
        H = (H + 2 * p - k) // s + 1
        out.append((co, H, period))
    return out


# ---- models/losses.py:475-623 ----

def feature_matching_loss(real_maps, fake_maps):
    """compute_feature_matching_loss: (total, [per discriminator])."""
    per = []
    for rl, fl in zip(real_maps, fake_maps):
        d = 0.0
        for r, f in zip(rl, fl):
            d = d + F.l1_loss(f, r)
        per.append(d / len(rl))
    return sum(per) / len(per), per


def discriminator_loss(real_outputs, fake_outputs):
    """compute_discriminator_loss"""
    loss = 0.0
    for dr, df in zip(real_outputs, fake_outputs):
        loss = loss + torch.mean((dr - 1.0) ** 2) + torch.mean(df ** 2)
    return loss / len(real_outputs)


def generator_adversarial_loss(fake_outputs):
    """compute_generator_adversarial_loss"""
    loss = 0.0
    for df in fake_outputs:
        loss = loss + torch.mean((df - 1.0) ** 2)
    return loss / len(fake_outputs)
