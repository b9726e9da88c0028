"""The reference's discriminators on the HIP device, forward only.

Mirrors ``models/hifigan.py`` of terrense/TTS-sambert_hifiGAN:

* ``ScaleDiscriminator``        models/hifigan.py:286-353
* ``MultiScaleDiscriminator``   models/hifigan.py:356-447
* ``PeriodDiscriminator``       models/hifigan.py:450-542
* ``MultiPeriodDiscriminator``  models/hifigan.py:545-615

Same constructor arguments, same submodule tree, same ``state_dict`` keys (legacy weight norm:
``weight_g`` / ``weight_v`` on every conv; Conv2d weights ``[C_out, C_in, k, 1]``), so a
reference state dict loads with ``strict=True``.  ``forward(x[B, 1, T])`` returns what the
reference returns: ``(output, feature_maps)``, or lists of those for the multi classes, as
float32 tensors of the reference's shapes on the device.  Each feature map is written once, in
that layout, by the kernels of ``disc_conv.hip`` / ``disc_thin.hip`` through the C ABI of
``include/hifigan_hip_disc.h``.

Critics, not a training step: no gradients (an input that requires grad under grad mode
raises), no spectral norm (``use_spectral_norm=True`` raises at construction), no CPU fallback
(a CPU tensor raises).  The parameters stay in ordinary ``nn.Conv1d`` / ``nn.Conv2d``
containers and are folded (``g v / |v|``), packed and uploaded again whenever one of them
changes (``hifigan._HipWeights``).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_int64, c_void_p
from typing import Dict, List, Tuple

import torch
import torch.nn as nn

from . import _lib
from ._frontend import check
from .hifigan import _HipWeights, _check_batch, get_padding


class DiscHandle:
    """Owning wrapper of an ``hfg_disc_handle*``: one discriminator on one device (``device``
    -1: host-only, shapes and sizes).  ``set_weight`` takes the module's parameters under
    their state-dict keys; ``commit`` folds weight norm and hands the C ABI folded tensors."""

    def __init__(self, kind: str, arg: int, device: int):
        self.lib = _lib.load_library()
        self.kind, self.arg, self.device = kind, int(arg), int(device)
        h = c_void_p()
        check(self.lib, self.lib.hfg_disc_create(_lib.DISC_KINDS[kind], int(arg), int(device),
                                                 ctypes.byref(h)))
        self.ptr = h
        self.num_maps = int(self.lib.hfg_disc_num_maps(h))
        self._pending: Dict[str, torch.Tensor] = {}

    def __del__(self):
        try:
            if getattr(self, "ptr", None):
                self.lib.hfg_disc_destroy(self.ptr)
                self.ptr = None
        except Exception:
            pass

    def set_weight(self, name: str, t: torch.Tensor):
        self._pending[name] = t.detach()

    def set_folded(self, key: str, t: torch.Tensor):
        """One folded tensor under the reference's name (``hfg_disc_set_weight``)."""
        t = t.detach().to(torch.float32).cpu().contiguous()
        shape = (c_int64 * max(t.dim(), 1))(*t.shape)
        check(self.lib, self.lib.hfg_disc_set_weight(self.ptr, key.encode(),
                                                     c_void_p(t.data_ptr()), shape, t.dim()))

    def commit(self):
        p, self._pending = self._pending, {}
        for key, t in p.items():
            if key.endswith(".weight_g"):
                continue
            if key.endswith(".weight_v"):
                mod = key[:-len(".weight_v")]
                g = p[mod + ".weight_g"].to(torch.float32)
                v = t.to(torch.float32)
                # the op the reference's weight-norm hook runs at forward time
                self.set_folded(mod + ".weight", torch._weight_norm(v, g, 0))
            else:
                self.set_folded(key, t)
        check(self.lib, self.lib.hfg_disc_commit(self.ptr))

    def map_shape(self, T: int, i: int) -> Tuple[int, int, int]:
        dims = (c_int64 * 3)()
        check(self.lib, self.lib.hfg_disc_map_shape(self.ptr, int(T), int(i), dims))
        return int(dims[0]), int(dims[1]), int(dims[2])

    def map_shapes(self, T: int) -> List[Tuple[int, int, int]]:
        return [self.map_shape(T, i) for i in range(self.num_maps)]

    def workspace_bytes(self, B: int, T: int) -> int:
        return int(self.lib.hfg_disc_workspace_bytes(self.ptr, int(B), int(T)))

    def fm_workspace_bytes(self, B: int) -> int:
        return int(self.lib.hfg_disc_fm_workspace_bytes(self.ptr, int(B)))

    def forward(self, wav_ptr: int, B: int, T: int, map_ptrs, ws_ptr: int, ws_bytes: int,
                stream: int):
        arr = (c_void_p * len(map_ptrs))(*[p if p else None for p in map_ptrs])
        check(self.lib, self.lib.hfg_disc_forward(
            self.ptr, c_void_p(wav_ptr) if wav_ptr else None, int(B), int(T), arr,
            c_void_p(ws_ptr) if ws_ptr else None, int(ws_bytes), c_void_p(stream)))

    def fm_sums(self, B: int, T: int, real_ptrs, fake_ptrs, sums_ptr: int, ws_ptr: int,
                ws_bytes: int, stream: int):
        r = (c_void_p * len(real_ptrs))(*[p if p else None for p in real_ptrs])
        f = (c_void_p * len(fake_ptrs))(*[p if p else None for p in fake_ptrs])
        check(self.lib, self.lib.hfg_disc_fm_sums(
            self.ptr, int(B), int(T), r, f, c_void_p(sums_ptr) if sums_ptr else None,
            c_void_p(ws_ptr) if ws_ptr else None, int(ws_bytes), c_void_p(stream)))

    def unpacked(self, layer: int, plane: int, numel: int):
        """Layer ``layer``'s packed weights read back through the layout (inspection)."""
        import numpy as np
        out = np.zeros(numel, dtype=np.float32)
        check(self.lib, self.lib.hfg_disc_debug_unpacked(
            self.ptr, int(layer), int(plane), out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
            out.size))
        return out


def _refuse_spectral_norm(flag: bool) -> None:
    if flag:
        raise NotImplementedError("spectral norm is out of scope for the MI355X discriminators; "
                                  "use_spectral_norm must be False")


class _Discriminator(_HipWeights):
    """What the two single discriminators share: weight tracking, the input rules, the call."""

    _kind = ""
    _arg = 0

    def _hip_weight_slots(self):
        for name, mod in [(f"convs.{i}", c) for i, c in enumerate(self.convs)] + \
                         [("conv_post", self.conv_post)]:
            names = (("weight_g", "weight_v") if hasattr(mod, "weight_g") and hasattr(mod, "weight_v")
                     else ("weight",))
            for p in names + ("bias",):
                yield name + "." + p, mod, p

    def _hip_new_handle(self, idx: int) -> DiscHandle:
        return DiscHandle(self._kind, self._arg, idx)

    def hip_handle(self, device) -> DiscHandle:
        """The committed handle of ``device``."""
        return self._handle_for(torch.device(device))

    def _check_input(self, x) -> torch.Tensor:
        name = type(self).__name__
        if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[1] != 1:
            raise RuntimeError(f"{name}: expected x [B, 1, T], got {getattr(x, 'shape', type(x))}")
        _check_batch(x.shape[0])
        if not x.is_cuda:
            raise RuntimeError(f"{name} (MI355X) runs on the HIP device only; move x to 'cuda' "
                               "(there is no CPU fallback)")
        if torch.is_grad_enabled() and x.requires_grad:
            raise NotImplementedError("forward-only HIP path: no autograd through the "
                                      "discriminators")
        if x.shape[0] == 0 or x.shape[2] == 0:
            raise RuntimeError("empty input")
        return x.detach().to(torch.float32).contiguous()

    def run(self, x: torch.Tensor) -> List[torch.Tensor]:
        """Every feature map of ``x`` [B, 1, T] (contiguous float32 on the device)."""
        B, _, T = x.shape
        with torch.cuda.device(x.device):
            h = self._handle_for(x.device)
            maps = [torch.empty((B,) + self._map_dims(s), dtype=torch.float32, device=x.device)
                    for s in h.map_shapes(T)]
            ws_bytes = h.workspace_bytes(B, T)
            ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=x.device)
            h.forward(x.data_ptr(), B, T, [m.data_ptr() for m in maps], ws.data_ptr(),
                      ws.numel(), torch.cuda.current_stream(x.device).cuda_stream)
        return maps

    def forward(self, x: torch.Tensor) -> Tuple[torch.Tensor, List[torch.Tensor]]:
        x = self._check_input(x)
        if self.debug_shapes:
            print(f"[{self._tag()}] Input shape: {x.shape}")
        maps = self.run(x)
        if self.debug_shapes:
            for i, m in enumerate(maps[:-1]):
                print(f"[{self._tag()}] After conv {i}: {m.shape}")
            print(f"[{self._tag()}] Output shape: {maps[-1].shape}")
            print(f"[{self._tag()}] Number of feature maps: {len(maps)}")
        return maps[-1], maps


class ScaleDiscriminator(_Discriminator):
    """models/hifigan.py:286-353.  ``_pools`` (0, 1 or 2, set by MultiScaleDiscriminator) is the
    number of ``AvgPool1d(4, 2, padding=2)`` the handle runs in front of ``convs.0``."""

    _kind = "scale"

    def __init__(self, use_spectral_norm: bool = False, debug_shapes: bool = False):
        super().__init__()
        _refuse_spectral_norm(use_spectral_norm)
        self.debug_shapes = debug_shapes or os.getenv("DEBUG_SHAPES", "0") == "1"
        norm_f = nn.utils.weight_norm
        self.convs = nn.ModuleList([
            norm_f(nn.Conv1d(1, 128, kernel_size=15, stride=1, padding=7)),
            norm_f(nn.Conv1d(128, 128, kernel_size=41, stride=2, groups=4, padding=20)),
            norm_f(nn.Conv1d(128, 256, kernel_size=41, stride=2, groups=16, padding=20)),
            norm_f(nn.Conv1d(256, 512, kernel_size=41, stride=4, groups=16, padding=20)),
            norm_f(nn.Conv1d(512, 1024, kernel_size=41, stride=4, groups=16, padding=20)),
            norm_f(nn.Conv1d(1024, 1024, kernel_size=41, stride=1, groups=16, padding=20)),
            norm_f(nn.Conv1d(1024, 1024, kernel_size=5, stride=1, padding=2)),
        ])
        self.conv_post = norm_f(nn.Conv1d(1024, 1, kernel_size=3, stride=1, padding=1))
        self._arg = 0
        self._hip_setup("f16x3")   # the one arithmetic disc_conv.hip runs

    def _tag(self):
        return "ScaleDiscriminator"

    @staticmethod
    def _map_dims(s):
        return (s[0], s[1])            # [B, C, L]


class MultiScaleDiscriminator(nn.Module):
    """models/hifigan.py:356-447: three ScaleDiscriminators on the wave, its 2x and its 4x
    average pooling.  The pooling runs inside each discriminator's forward."""

    def __init__(self, use_spectral_norm: bool = False, debug_shapes: bool = False):
        super().__init__()
        _refuse_spectral_norm(use_spectral_norm)
        self.debug_shapes = debug_shapes or os.getenv("DEBUG_SHAPES", "0") == "1"
        self.discriminators = nn.ModuleList([
            ScaleDiscriminator(use_spectral_norm, debug_shapes) for _ in range(3)])
        for i, d in enumerate(self.discriminators):
            d._arg = i
        # parameter-free, kept for the reference's module tree (the kernels pool)
        self.poolings = nn.ModuleList([
            nn.Identity(),
            nn.AvgPool1d(kernel_size=4, stride=2, padding=2),
            nn.AvgPool1d(kernel_size=4, stride=2, padding=2)])

    def forward(self, x: torch.Tensor) -> Tuple[List[torch.Tensor], List[List[torch.Tensor]]]:
        if self.debug_shapes:
            print(f"[MultiScaleDiscriminator] Input shape: {x.shape}")
        outputs, feature_maps_list = [], []
        for i, disc in enumerate(self.discriminators):
            output, feature_maps = disc(x)
            outputs.append(output)
            feature_maps_list.append(feature_maps)
            if self.debug_shapes:
                print(f"[MultiScaleDiscriminator] Scale {i} output shape: {output.shape}")
        return outputs, feature_maps_list


class PeriodDiscriminator(_Discriminator):
    """models/hifigan.py:450-542; ``kernel_size`` 5 and ``stride`` 3 are the ones built."""

    _kind = "period"

    def __init__(self, period: int, kernel_size: int = 5, stride: int = 3,
                 use_spectral_norm: bool = False, debug_shapes: bool = False):
        super().__init__()
        _refuse_spectral_norm(use_spectral_norm)
        if kernel_size != 5 or stride != 3:
            raise NotImplementedError("PeriodDiscriminator (MI355X): kernel_size 5 and stride 3 "
                                      "only (the reference's)")
        if int(period) < 1:
            raise ValueError(f"period must be >= 1, got {period!r}")
        self.period = int(period)
        self.debug_shapes = debug_shapes or os.getenv("DEBUG_SHAPES", "0") == "1"
        norm_f = nn.utils.weight_norm
        pad = (get_padding(kernel_size, 1), 0)
        self.convs = nn.ModuleList([
            norm_f(nn.Conv2d(1, 32, kernel_size=(kernel_size, 1), stride=(stride, 1), padding=pad)),
            norm_f(nn.Conv2d(32, 128, kernel_size=(kernel_size, 1), stride=(stride, 1), padding=pad)),
            norm_f(nn.Conv2d(128, 512, kernel_size=(kernel_size, 1), stride=(stride, 1), padding=pad)),
            norm_f(nn.Conv2d(512, 1024, kernel_size=(kernel_size, 1), stride=(stride, 1), padding=pad)),
            norm_f(nn.Conv2d(1024, 1024, kernel_size=(kernel_size, 1), stride=1, padding=(2, 0))),
        ])
        self.conv_post = norm_f(nn.Conv2d(1024, 1, kernel_size=(3, 1), stride=1, padding=(1, 0)))
        self._arg = self.period
        self._hip_setup("f16x3")   # the one arithmetic disc_conv.hip runs

    def _tag(self):
        return f"PeriodDiscriminator-{self.period}"

    @staticmethod
    def _map_dims(s):
        return tuple(s)                # [B, C, H, period]


class MultiPeriodDiscriminator(nn.Module):
    """models/hifigan.py:545-615."""

    def __init__(self, periods: List[int] = [2, 3, 5, 7, 11], use_spectral_norm: bool = False,
                 debug_shapes: bool = False):
        super().__init__()
        _refuse_spectral_norm(use_spectral_norm)
        self.debug_shapes = debug_shapes or os.getenv("DEBUG_SHAPES", "0") == "1"
        self.periods = periods
        self.discriminators = nn.ModuleList([
            PeriodDiscriminator(p, use_spectral_norm=use_spectral_norm, debug_shapes=debug_shapes)
            for p in periods])

    def forward(self, x: torch.Tensor) -> Tuple[List[torch.Tensor], List[List[torch.Tensor]]]:
        if self.debug_shapes:
            print(f"[MultiPeriodDiscriminator] Input shape: {x.shape}")
        outputs, feature_maps_list = [], []
        for i, disc in enumerate(self.discriminators):
            output, feature_maps = disc(x)
            outputs.append(output)
            feature_maps_list.append(feature_maps)
            if self.debug_shapes:
                print(f"[MultiPeriodDiscriminator] Period {self.periods[i]} output shape: "
                      f"{output.shape}")
        return outputs, feature_maps_list


def single_discriminators(discs) -> List[_Discriminator]:
    """The single discriminators of ``discs`` in the reference's order (MSD's, then MPD's): a
    single one, an MSD, an MPD, a ``HiFiGAN`` built with ``discriminators=True``, or a list."""
    from .hifigan import HiFiGAN
    if isinstance(discs, _Discriminator):
        return [discs]
    if isinstance(discs, (MultiScaleDiscriminator, MultiPeriodDiscriminator)):
        return list(discs.discriminators)
    if isinstance(discs, HiFiGAN):
        if discs.msd is None or discs.mpd is None:
            raise RuntimeError("this HiFiGAN was built without discriminators; pass "
                               "discriminators=True to its constructor")
        return list(discs.msd.discriminators) + list(discs.mpd.discriminators)
    if isinstance(discs, (list, tuple)) and discs:
        return [s for d in discs for s in single_discriminators(d)]
    raise TypeError("expected a discriminator, an MSD, an MPD, a HiFiGAN(discriminators=True) "
                    f"or a list of those, got {type(discs).__name__}")
