"""MI355X-native HiFi-GAN Generator inference path (drop-in for
terrense/TTS-sambert_hifiGAN ``models/hifigan.py`` Generator.forward).

The directory name contains a hyphen, so import it with :func:`load_package`
from the repo root (``__graft_entry__``, ``bench.py`` and ``tests/conftest.py``
do this), which registers it as ``tts_sambert_hifigan_amd``.
"""
from .hifigan import (HiFiGAN, HiFiGANGenerator, MRF, ResBlock, ResBlock2,  # noqa: F401
                      get_padding)
from ._lib import (HipExtensionMissing, HfgError, Handle, load_library, make_config,  # noqa: F401
                   LIB_PATH, check_provenance, schedule_override, schedule_clear,
                   schedule_overrides)
from . import pcm  # noqa: F401  (the release's PCM boundary: pcm.peak / to_float / to_pcm16)
from . import metrics  # noqa: F401  (spectral distances: metrics.mel_distance / MultiResolutionSTFT)
from . import discriminators  # noqa: F401  (the reference's MSD / MPD, forward only)

__all__ = ["HiFiGAN", "HiFiGANGenerator", "MRF", "ResBlock", "ResBlock2", "get_padding", "Handle",
           "HipExtensionMissing", "HfgError", "load_library", "make_config", "LIB_PATH", "check_provenance",
           "schedule_override", "schedule_clear", "schedule_overrides", "pcm", "metrics"]
