"""Forward-only spectral distances on the HIP device: how well a waveform realises a mel.

The two discriminator-free terms of the reference's ``VocoderLoss`` (``models/losses.py``) as
metrics, with no gradients and no host round trip:

* :func:`mel_distance` — ``mel_reconstruction_loss`` (:708-797) in the form that needs no
  ground-truth audio: the mel of ``wav`` (by a :class:`mel.ReleaseMelSpectrogram` or a
  :class:`mel.MelSpectrogram`) against a mel tensor already held (the mel fed to the
  Generator, an acoustic model's prediction, the front end's output in copy-synthesis).  With
  the release front end and ``target = mel_spectrogram(y)`` it is the release training loop's
  validation error ``F.l1_loss(y_mel, mel_spectrogram(y_g_hat))``.
* :class:`MultiResolutionSTFT` — ``compute_stft_loss`` (:625-706): mean ``|d|`` and mean
  ``d²`` of ``d = ln(|STFT a| + 1e-5) − ln(|STFT b| + 1e-5)`` over three resolutions.

The remaining two terms need the model's own critics (``discriminators.py``):
:func:`feature_matching` (``compute_feature_matching_loss``, :537-623) and
:func:`discriminator_scores` (the pieces of ``compute_discriminator_loss`` /
``compute_generator_adversarial_loss``, :475-535), from float64 sums formed without atomics.

The spectral distances run in ``spectral_distance.hip`` (float64 FFT, float64 sums, no atomics): results are
bitwise reproducible, item b of a ragged batch is bitwise its solo run, and the calls are
capturable.  There is no CPU fallback: a CPU tensor raises.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._frontend import (HandleOwner, check, float_ptr, lengths as _lengths, ptr as _ptr,
                        stream as _stream)

REFERENCE_RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))


class SpectralDistance:
    """Per-item sums of one distance, device tensors only: ``sum_abs`` = Σ|d| and ``sum_sq`` =
    Σd² (float64 ``[B]``), ``frames`` (int32 ``[B]``, the frames compared) and ``rows`` (entries
    per frame: n_mels, or n_fft/2 + 1 for an STFT).  Nothing here reads a value back."""

    def __init__(self, sum_abs: torch.Tensor, sum_sq: torch.Tensor, frames: torch.Tensor,
                 rows: int):
        self.sum_abs, self.sum_sq, self.frames, self.rows = sum_abs, sum_sq, frames, int(rows)

    def _per_item(self, s):
        return s / (self.rows * self.frames.clamp(min=1).to(torch.float64))

    @property
    def per_item_l1(self) -> torch.Tensor:
        """Mean |d| of each item, float64 [B]; 0 for an item without frames."""
        return self._per_item(self.sum_abs)

    @property
    def per_item_l2(self) -> torch.Tensor:
        """Mean d² of each item, float64 [B]; 0 for an item without frames."""
        return self._per_item(self.sum_sq)

    def _batch(self, s):
        return s.sum() / (self.rows * self.frames.sum().clamp(min=1).to(torch.float64))

    @property
    def l1(self) -> torch.Tensor:
        """Σ sums / (rows · Σ frames): ``F.l1_loss`` on a batch that is not ragged."""
        return self._batch(self.sum_abs)

    @property
    def l2(self) -> torch.Tensor:
        """``F.mse_loss`` on a batch that is not ragged."""
        return self._batch(self.sum_sq)


def _wav_rows(wav, what: str) -> torch.Tensor:
    if not (isinstance(wav, torch.Tensor) and wav.is_cuda):
        raise RuntimeError(f"{what} (MI355X) needs a HIP tensor; no CPU fallback")
    if wav.dim() == 3 and wav.shape[1] == 1:
        wav = wav[:, 0]
    if wav.dim() != 2 or wav.shape[0] < 1:
        raise RuntimeError(f"{what}: expected wav [B, N] or [B, 1, N], got {tuple(wav.shape)}")
    return wav.detach().to(torch.float32).contiguous()


def _outputs(B: int, ws_bytes: int, device):
    sums = torch.empty(B, 2, dtype=torch.float64, device=device)
    frames = torch.empty(B, dtype=torch.int32, device=device)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=device)
    return sums, frames, ws


def mel_distance(frontend, wav: torch.Tensor, target: torch.Tensor, lengths=None
                 ) -> SpectralDistance:
    """The mel of ``wav`` ([B, N] or [B, 1, N] on the HIP device) by ``frontend`` against
    ``target`` [B, n_mels, T] float32: Σ|d| and Σd² per item in one fused launch plus a small
    reduction; the mel itself is never written.  ``d`` uses the float32 value the front end
    would have stored.  Item b compares ``min(frames(lengths[b]), T)`` frames, framed as if it
    were alone; samples past its length and target columns past its frames are never read.
    ``lengths``: None, a sequence of ints or an int tensor [B]; host values are validated (in
    ``[0, N]``), a device tensor is never read back (the kernel clamps it)."""
    from . import mel as _mel
    if isinstance(frontend, _mel.ReleaseMelSpectrogram):
        fn, ws_fn, rows = "hfg_relmel_distance", "hfg_relmel_distance_workspace_bytes", frontend.num_mels
    elif isinstance(frontend, _mel.MelSpectrogram):
        fn, ws_fn, rows = "hfg_mel_distance", "hfg_mel_distance_workspace_bytes", frontend.n_mels
    else:
        raise TypeError("mel_distance: frontend must be a mel.ReleaseMelSpectrogram or a "
                        "mel.MelSpectrogram")
    wav = _wav_rows(wav, "mel_distance")
    B, N = wav.shape
    if not (isinstance(target, torch.Tensor) and target.is_cuda):
        raise RuntimeError("mel_distance (MI355X) needs a HIP target tensor; no CPU fallback")
    if target.dim() != 3 or target.shape[0] != B or target.shape[1] != rows or target.shape[2] < 1:
        raise RuntimeError(f"mel_distance: expected target [{B}, {rows}, T >= 1], got "
                           f"{tuple(target.shape)}")
    if target.device != wav.device:
        raise RuntimeError("mel_distance: wav and target are on different devices")
    target = target.detach().to(torch.float32).contiguous()
    lens_t = _lengths(lengths, B, N, wav.device)
    lib = frontend.lib
    ws_bytes = int(getattr(lib, ws_fn)(frontend.ptr, B, N))
    sums, frames, ws = _outputs(B, ws_bytes, wav.device)
    with torch.cuda.device(wav.device):
        check(lib, getattr(lib, fn)(frontend.ptr, _ptr(wav), B, N, _ptr(lens_t), _ptr(target),
                                    target.shape[2], _ptr(ws), ws.numel(), _ptr(sums),
                                    _ptr(frames), _stream(wav.device)))
    return SpectralDistance(sums[:, 0], sums[:, 1], frames, rows)


class _StftDistance(HandleOwner):
    """One resolution (``hfg_stftdist_*``)."""

    def __init__(self, n_fft: int, hop_length: int, win_length: int, eps: float, device=None):
        c = _lib.HfgStftdistConfig(int(n_fft), int(hop_length), int(win_length), float(eps))
        self.n_fft, self.hop_length, self.win_length = int(n_fft), int(hop_length), int(win_length)
        self._open("hfg_stftdist_create", "hfg_stftdist_destroy", ctypes.byref(c), device=device)
        # torch.stft's own float32 window (the reference's torch.hann_window(win), centred)
        from .mel import stft_window
        self._window = stft_window(self.n_fft, self.win_length).contiguous()
        check(self.lib, self.lib.hfg_stftdist_set_window(self.ptr, float_ptr(self._window)))

    def __call__(self, a, b, lens_t) -> SpectralDistance:
        B, N = a.shape
        ws_bytes = int(self.lib.hfg_stftdist_workspace_bytes(self.ptr, B, N))
        sums, frames, ws = _outputs(B, ws_bytes, a.device)
        with torch.cuda.device(a.device):
            check(self.lib, self.lib.hfg_stftdist_forward(
                self.ptr, _ptr(a), _ptr(b), B, N, _ptr(lens_t), _ptr(ws), ws.numel(), _ptr(sums),
                _ptr(frames), _stream(a.device)))
        return SpectralDistance(sums[:, 0], sums[:, 1], frames, self.n_fft // 2 + 1)


class MultiResolutionSTFTResult(list):
    """One :class:`SpectralDistance` per resolution; ``l1`` / ``l2`` are the reference's
    ``sc_loss`` / ``mag_loss``: the mean over resolutions of each resolution's batch mean
    (0-dim float64 device tensors)."""

    @property
    def l1(self) -> torch.Tensor:
        return torch.stack([d.l1 for d in self]).mean()

    @property
    def l2(self) -> torch.Tensor:
        return torch.stack([d.l2 for d in self]).mean()


class MultiResolutionSTFT:
    """The reference's multi-resolution STFT distance (``VocoderLoss.compute_stft_loss``) on the
    HIP device: per resolution ``(n_fft, hop, win)`` one launch over both signals,
    ``torch.stft(center=True)`` framing with the periodic Hann window, float64 FFT,
    ``ln(|X| + eps)`` rounded to float32 on each side as the reference holds it.  ``n_fft`` must
    be a power of two in [16, 2048]."""

    def __init__(self, resolutions: Sequence[Tuple[int, int, int]] = REFERENCE_RESOLUTIONS,
                 eps: float = 1e-5, device=None):
        if not resolutions:
            raise ValueError("MultiResolutionSTFT: at least one resolution")
        self.resolutions = tuple(tuple(int(v) for v in r) for r in resolutions)
        # 1e-5 goes as 0: the library's own default, the double 1e-5 (not its float32 rounding)
        self._dists: List[_StftDistance] = [
            _StftDistance(n, h, w, 0.0 if eps == 1e-5 else eps, device=device)
            for n, h, w in self.resolutions]

    def __call__(self, a: torch.Tensor, b: torch.Tensor, lengths=None
                 ) -> MultiResolutionSTFTResult:
        """a, b: [B, N] or [B, 1, N] on the HIP device, sharing ``lengths`` (as
        :func:`mel_distance`).  Item b has ``lengths[b] // hop + 1`` frames at a resolution when
        ``lengths[b] > n_fft / 2``, else 0."""
        a = _wav_rows(a, "MultiResolutionSTFT")
        b = _wav_rows(b, "MultiResolutionSTFT")
        if a.shape != b.shape or a.device != b.device:
            raise RuntimeError(f"MultiResolutionSTFT: a {tuple(a.shape)} and b {tuple(b.shape)} "
                               "must have one shape and one device")
        lens_t = _lengths(lengths, a.shape[0], a.shape[1], a.device)
        return MultiResolutionSTFTResult(d(a, b, lens_t) for d in self._dists)


# ---------------------------------------------------------------------------------------------
# The model's own critics (discriminators.py): the remaining VocoderLoss terms as metrics.


class FeatureMatching:
    """``compute_feature_matching_loss`` (models/losses.py:595-623) as numbers, all float64 on
    the device: ``per_discriminator`` [D] (per discriminator the mean over its layers of the
    batch mean |fake - real|), ``total`` (their mean, 0-dim) and ``per_item`` [B] (the same
    formula restricted to item b; bitwise item b's solo value)."""

    def __init__(self, per_discriminator, total, per_item):
        self.per_discriminator, self.total, self.per_item = per_discriminator, total, per_item


def _critic_wav(wav, what: str) -> torch.Tensor:
    if not (isinstance(wav, torch.Tensor) and wav.is_cuda):
        raise RuntimeError(f"{what} (MI355X) needs a HIP tensor; no CPU fallback")
    if wav.dim() == 2:
        wav = wav[:, None]
    if wav.dim() != 3 or wav.shape[1] != 1 or wav.shape[0] < 1 or wav.shape[2] < 1:
        raise RuntimeError(f"{what}: expected wav [B, 1, T] or [B, T], got {tuple(wav.shape)}")
    if torch.is_grad_enabled() and wav.requires_grad:
        raise NotImplementedError("forward-only HIP path: no autograd through the discriminators")
    return wav.detach().to(torch.float32).contiguous()


def feature_matching(discs, wav_real: torch.Tensor, wav_fake: torch.Tensor) -> FeatureMatching:
    """The feature-matching distance of two waveforms under ``discs`` (an MSD, an MPD, a single
    discriminator, a ``HiFiGAN(discriminators=True)`` or a list of those).  Real and fake run as
    one batch of 2B through each discriminator; ``hfg_disc_fm_sums`` then adds |fake - real|
    per (item, map) in float64 with no atomics and a fixed order.  Nothing is read back."""
    from .discriminators import single_discriminators
    singles = single_discriminators(discs)
    real = _critic_wav(wav_real, "feature_matching")
    fake = _critic_wav(wav_fake, "feature_matching")
    if real.shape != fake.shape or real.device != fake.device:
        raise RuntimeError(f"feature_matching: wav_real {tuple(real.shape)} and wav_fake "
                           f"{tuple(fake.shape)} must have one shape and one device")
    B, _, T = real.shape
    dev = real.device
    both = torch.cat([real, fake], dim=0)
    per_disc, per_item = [], None
    with torch.cuda.device(dev):
        for d in singles:
            d._check_input(both)
            maps = d.run(both)
            h = d.hip_handle(dev)
            sums = torch.empty(B, len(maps), dtype=torch.float64, device=dev)
            ws = torch.empty(max(h.fm_workspace_bytes(B), 16), dtype=torch.uint8, device=dev)
            h.fm_sums(B, T, [m.data_ptr() for m in maps], [m[B:].data_ptr() for m in maps],
                      sums.data_ptr(), ws.data_ptr(), ws.numel(),
                      torch.cuda.current_stream(dev).cuda_stream)
            # layer means in layer order, elementwise per item: no reduction whose order could
            # depend on the batch
            item = None
            for i, m in enumerate(maps):
                term = sums[:, i] / float(m[0].numel())
                item = term if item is None else item + term
            item = item / float(len(maps))
            per_disc.append(item.sum() / float(B))
            per_item = item if per_item is None else per_item + item
    per_disc_t = torch.stack(per_disc)
    total = per_disc[0]
    for v in per_disc[1:]:
        total = total + v
    return FeatureMatching(per_disc_t, total / float(len(singles)), per_item / float(len(singles)))


class DiscriminatorScores:
    """Per discriminator, over its whole score map: ``sq`` = mean d² and ``sq_minus_one`` =
    mean (d - 1)² (float64 [D] on the device) — the pieces of the reference's LSGAN terms
    (models/losses.py:475-535)."""

    def __init__(self, sq: torch.Tensor, sq_minus_one: torch.Tensor):
        self.sq, self.sq_minus_one = sq, sq_minus_one

    @property
    def generator_adversarial(self) -> torch.Tensor:
        """``compute_generator_adversarial_loss`` of these (fake) scores."""
        return self.sq_minus_one.sum() / float(self.sq_minus_one.numel())

    @staticmethod
    def discriminator_loss(real: "DiscriminatorScores", fake: "DiscriminatorScores"
                           ) -> torch.Tensor:
        """``compute_discriminator_loss``: the mean over discriminators of
        mean (D(real) - 1)² + mean D(fake)²."""
        return (real.sq_minus_one + fake.sq).sum() / float(fake.sq.numel())


def discriminator_scores(discs, wav: torch.Tensor) -> DiscriminatorScores:
    """The scores of ``wav`` [B, 1, T] under every single discriminator of ``discs``."""
    from .discriminators import single_discriminators
    singles = single_discriminators(discs)
    x = _critic_wav(wav, "discriminator_scores")
    sq, sq1 = [], []
    with torch.cuda.device(x.device):
        for d in singles:
            d._check_input(x)
            s = d.run(x)[-1].to(torch.float64)
            sq.append((s * s).mean())
            sq1.append(((s - 1.0) * (s - 1.0)).mean())
    return DiscriminatorScores(torch.stack(sq), torch.stack(sq1))
