"""Record the REFERENCE's multi-resolution STFT loss on the shared inputs into
tests/golden/specdist_ref.json.

    python tests/golden/make_specdist_golden.py REFERENCE_CHECKOUT

Needs a checkout of the reference (terrense/TTS-sambert_hifiGAN), read-only.  Its
``VocoderLoss.compute_stft_loss`` (models/losses.py:625-706) is called unbound on a stub that
carries only ``stft_params``, so nothing else of the class (torchaudio's MelSpectrogram among
it) is constructed.  The inputs are regenerated from code (spectral_distance_oracle.inputs);
the file holds the reference's float32 ``(sc_loss, mag_loss)`` per resolution and over all
three, the float64 oracle's values beside them, and their measured differences: the margin of
tests/test_spectral_distance_host.py is 4 x those (the reference's own float32 FFT noise at
quiet bins; not derivable).  Nothing of the reference's program text is stored.
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
OUT = os.path.join(HERE, "specdist_ref.json")


def main(ref_dir):
    import spectral_distance_oracle as O
    sys.path.insert(0, ref_dir)
    os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
    from models.losses import VocoderLoss  # the reference

    a, b = O.inputs()

    def ref_loss(resolutions):
        stub = types.SimpleNamespace(stft_params=[
            dict(n_fft=n, hop_length=h, win_length=w) for n, h, w in resolutions])
        sc, mag = VocoderLoss.compute_stft_loss(stub, a[:, None], b[:, None])
        return float(sc), float(mag)

    def oracle_loss(r):
        s1, s2, fr = O.stft_distance64(a, b, *r)
        return O.means(s1, s2, fr, r[0] // 2 + 1)[2:]

    rec = {"inputs": "spectral_distance_oracle.inputs(8269): a [3, 8269], b = 0.9 a + 0.01 randn(seed 7)",
           "reference": "models/losses.py VocoderLoss.compute_stft_loss, float32, imported read-only",
           "resolutions": []}
    o1s, o2s = [], []
    for r in O.RESOLUTIONS:
        sc, mag = ref_loss([r])
        o1, o2 = oracle_loss(r)
        o1s.append(o1)
        o2s.append(o2)
        rec["resolutions"].append({"n_fft": r[0], "hop": r[1], "win": r[2], "sc_loss": sc,
                                   "mag_loss": mag, "oracle_l1": o1, "oracle_l2": o2,
                                   "diff_l1": abs(sc - o1), "diff_l2": abs(mag - o2)})
    sc, mag = ref_loss(O.RESOLUTIONS)
    o1, o2 = float(np.mean(o1s)), float(np.mean(o2s))
    rec["overall"] = {"sc_loss": sc, "mag_loss": mag, "oracle_l1": o1, "oracle_l2": o2,
                      "diff_l1": abs(sc - o1), "diff_l2": abs(mag - o2)}
    every = rec["resolutions"] + [rec["overall"]]
    rec["measured_max_diff"] = {"l1": max(e["diff_l1"] for e in every),
                                "l2": max(e["diff_l2"] for e in every)}
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["measured_max_diff"]))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
