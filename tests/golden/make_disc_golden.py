"""Record the REFERENCE's discriminator feature maps and loss values on the shared weights and
inputs into tests/golden/disc_*.npz, disc_loss_ref.json and disc_index.json.

    python tests/golden/make_disc_golden.py REFERENCE_CHECKOUT

Needs a checkout of the reference (terrense/TTS-sambert_hifiGAN), read-only.  The state dicts
of tests/disc_cases.py are loaded (strict) into the reference's own ``PeriodDiscriminator(3)``,
``PeriodDiscriminator(11)``, ``ScaleDiscriminator``, ``MultiScaleDiscriminator`` and
``MultiPeriodDiscriminator`` (models/hifigan.py:286-616) and run in float32 on the PRNG inputs
with B = 1:

  disc_period3_t730.npz    the input and all 6 maps (pad 2; H 244 -> 82 -> 28 -> 10 -> 4)
  disc_period11_t100.npz   the input and all 6 maps (pad 10; H collapses to 1)
  disc_scale_t257.npz      the input and all 8 maps
  disc_msd_t257.npz        the input, the three entry maps and the three scores
  disc_loss_ref.json       compute_feature_matching_loss / compute_discriminator_loss /
                           compute_generator_adversarial_loss (models/losses.py:475-623),
                           called unbound on a stub, on the MSD + MPD maps of the pair
                           real, fake = 0.9 real + 0.01 randn (disc_cases.loss_pair)
  disc_index.json          state-dict keys and shapes of the four reference modules

Only outputs are stored; nothing of the reference's program text.
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main(ref_dir):
    import torch
    import disc_cases as DC
    sys.path.insert(0, ref_dir)
    os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
    sys.dont_write_bytecode = True
    from models import hifigan as R          # the reference
    from models.losses import VocoderLoss

    def save(name, x, maps):
        path = os.path.join(HERE, name)
        np.savez(path, x=x.numpy(), **{f"map{i}": m.numpy() for i, m in enumerate(maps)})
        assert os.path.getsize(path) < 512 * 1024, (name, os.path.getsize(path))

    index = {}

    def keys_of(name, module):
        index[name] = [[k, list(v.shape)] for k, v in module.state_dict().items()]

    with torch.no_grad():
        for p, T in ((3, 730), (11, 100)):
            d = R.PeriodDiscriminator(p)
            d.load_state_dict(DC.period_state(), strict=True)
            x = DC.wav(T)
            save(f"disc_period{p}_t{T}.npz", x, d(x)[1])
        keys_of("PeriodDiscriminator", d)

        d = R.ScaleDiscriminator()
        d.load_state_dict(DC.scale_state(), strict=True)
        keys_of("ScaleDiscriminator", d)
        x = DC.wav(257)
        save("disc_scale_t257.npz", x, d(x)[1])

        msd = R.MultiScaleDiscriminator()
        msd.load_state_dict(DC.msd_state_dict(), strict=True)
        keys_of("MultiScaleDiscriminator", msd)
        outs, feats = msd(x)
        save("disc_msd_t257.npz", x, [f[0] for f in feats] + list(outs))

        mpd = R.MultiPeriodDiscriminator()
        mpd.load_state_dict({f"discriminators.{i}.{k}": v for i, s in enumerate(DC.SEED_MPD)
                             for k, v in DC.period_state(s).items()}, strict=True)
        keys_of("MultiPeriodDiscriminator", mpd)

        real, fake = DC.loss_pair()
        ro_s, rf_s = msd(real)
        fo_s, ff_s = msd(fake)
        ro_p, rf_p = mpd(real)
        fo_p, ff_p = mpd(fake)
        stub = types.SimpleNamespace()
        fm, per = VocoderLoss.compute_feature_matching_loss(stub, rf_s + rf_p, ff_s + ff_p,
                                                            return_per_discriminator=True)
        rec = {"inputs": "disc_cases.loss_pair(257): real [1, 1, 257], fake = 0.9 real + 0.01 randn",
               "reference": "models/losses.py VocoderLoss, float32, imported read-only; maps of "
                            "the reference's MSD (seeds SEED_MSD) then MPD (seeds SEED_MPD)",
               "feature_matching": float(fm), "feature_matching_per_discriminator": per,
               "discriminator_loss": float(VocoderLoss.compute_discriminator_loss(
                   stub, ro_s + ro_p, fo_s + fo_p)),
               "generator_adversarial": float(VocoderLoss.compute_generator_adversarial_loss(
                   stub, fo_s + fo_p))}
    with open(os.path.join(HERE, "disc_loss_ref.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    with open(os.path.join(HERE, "disc_index.json"), "w") as f:
        json.dump(index, f)
        f.write("\n")
    print(json.dumps({k: v for k, v in rec.items() if isinstance(v, float)}))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
