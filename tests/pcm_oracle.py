"""CPU restatement of the public HiFi-GAN release's PCM boundary, numpy only.  TEST
INFRASTRUCTURE ONLY, not a test module.

* :func:`normalize_ref` — what ``meldataset.py`` hands ``mel_spectrogram``:
  ``audio / MAX_WAV_VALUE`` on an int16 array (float64), ``librosa.util.normalize`` (a float64
  division by ``max |.|``, a vector whose peak is below the dtype's smallest normal number left
  undivided), ``* 0.95`` (float64), ``torch.FloatTensor`` (one rounding).  librosa is not
  installed here; its rule is restated from the published definition.
* :func:`normalize_f32` — the same steps with every operand float32, the way a hand-written
  torch version evaluates them: NOT the release's values (test_pcm_host.py counts how many
  samples differ).
* :func:`quantize_ref` — ``sat16(round(x * 32768))``, the library's documented output stage
  (``inference.py``'s ``astype('int16')`` plus saturation).
* :func:`pcm_signals` — the int16 test batch.
"""
import numpy as np
import torch

from release_mel_oracle import signals

# the values the output stage must get right: both saturation edges, the largest float32
# below 1 on either side, the rounding ties and their neighbours, the non-finite values
SPECIALS = np.array([1.0, -1.0, 0.99999994, 0.5 / 32768, -0.5 / 32768, 1.5 / 32768,
                     -1.5 / 32768, np.nan, np.inf, -np.inf, -0.99999994], np.float32)
SPECIALS_TRUNC = np.array([32767, -32768, 32767, 0, 0, 1, -1, 0, 32767, -32768, -32767], np.int16)
SPECIALS_NEAREST = np.array([32767, -32768, 32767, 0, 0, 2, -2, 0, 32767, -32768, -32768], np.int16)


def pcm_signals(n):
    """int16 [3, n]: round(20000 * [tone + noise, chirp, their mean]) of
    release_mel_oracle.signals(n)."""
    s = signals(n)
    x = torch.stack([s[0], s[1], 0.5 * (s[0] + s[1])])
    return torch.round(x * 20000).to(torch.int16).numpy()


def peak_ref(s, n):
    """max |s[:n]| as the library's peak: float32, int16 magnitudes over 32768; 0 when n = 0."""
    s = np.asarray(s)[:n]
    if s.size == 0:
        return np.float32(0)
    if s.dtype == np.int16:
        return np.float32(np.abs(s.astype(np.int32)).max() / 32768.0)
    return np.float32(np.abs(s).max())


def normalize_ref(s, n, gain=0.95):
    """float32 [n]: ((s[:n] / 32768.0) / max|.| * gain) in float64, rounded once.  s int16, or
    float32 (then v = float64(s)); the divisor is 1 when the peak is below the smallest normal
    number of the vector's dtype (float64 for the int16 path, float32 for float32 input)."""
    s = np.asarray(s)[:n]
    if s.dtype == np.int16:
        v, tiny = s / 32768.0, np.finfo(np.float64).tiny
    else:
        assert s.dtype == np.float32
        v, tiny = s.astype(np.float64), np.finfo(np.float32).tiny
    assert v.dtype == np.float64
    peak = np.abs(v).max() if v.size else 0.0
    d = 1.0 if peak < tiny else peak
    return ((v / d) * np.float64(gain)).astype(np.float32)


def normalize_f32(s, n, gain=0.95):
    """The same steps evaluated in float32 throughout (int16 input)."""
    v = np.asarray(s)[:n].astype(np.float32) / np.float32(32768.0)
    peak = np.abs(v).max() if v.size else np.float32(0)
    d = np.float32(1.0) if peak < np.finfo(np.float32).tiny else peak
    out = (v / d) * np.float32(gain)
    assert out.dtype == np.float32
    return out


def quantize_ref(x, mode="trunc"):
    """int16: sat16(round(x * 32768)) of float32 x; "trunc" rounds toward zero, "nearest" to
    nearest even; NaN gives 0, +-inf and anything past the range saturate."""
    q = np.asarray(x, np.float32).astype(np.float64) * 32768.0   # exact
    q = np.trunc(q) if mode == "trunc" else np.rint(q)
    assert mode in ("trunc", "nearest")
    q = np.where(np.isnan(q), 0.0, np.clip(q, -32768.0, 32767.0))
    return q.astype(np.int16)
