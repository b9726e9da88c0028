#!/usr/bin/env python3
"""Time the device discriminators against PyTorch-ROCm's own conv path on the same GPU (needs
the GPU).

    python tests/tools/time_discriminators.py [--steps 20] [--warmup 3] [--step-limit 120]
                                              [--shapes 16x8192,8x262144]

Two shapes: a training segment, wav [16, 1, 8192], and whole utterances, wav [8, 1, 262144].
Per shape, in one process and alternating call by call: the MultiScaleDiscriminator and the
MultiPeriodDiscriminator forward of this package (disc_conv.hip / disc_thin.hip), the same two
as the ATen restatement of tests/discriminator_oracle.py in float32 on the same device (what
a user would otherwise run), and ``metrics.feature_matching`` over both against the ATen maps
plus ``F.l1_loss``.  Each call is bracketed by a HIP event pair behind a short device-side
spin, so the interval holds the kernels, not the host's launch path.  Median / min / p90 over
the timed steps after the warm-up; a step (warm-up included) that takes longer than
--step-limit seconds ends the run.  Prints one line per entry and one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-limit", type=float, default=120.0)
    ap.add_argument("--shapes", default="16x8192,8x262144")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_discriminators: no HIP device (a timing needs the GPU)")
    import __graft_entry__ as ge
    pkg = ge.load_package()
    pkg.check_provenance()
    import discriminator_oracle as DO
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    D = pkg.discriminators
    msd, mpd = D.MultiScaleDiscriminator().to(dev), D.MultiPeriodDiscriminator().to(dev)
    sub = lambda m: [{k: v.detach() for k, v in d.state_dict().items()} for d in m.discriminators]
    msd_sd, mpd_sd = sub(msd), sub(mpd)

    def aten_fm(real, fake):
        rm = DO.msd_forward(msd_sd, real) + DO.mpd_forward(mpd_sd, real)
        fm = DO.msd_forward(msd_sd, fake) + DO.mpd_forward(mpd_sd, fake)
        return DO.feature_matching_loss(rm, fm)[0]

    result = {}
    for shape in args.shapes.split(","):
        B, T = (int(v) for v in shape.split("x"))
        g = torch.Generator().manual_seed(B + T)
        real = (0.3 * torch.randn(B, 1, T, generator=g)).to(dev)
        fake = (0.9 * real + 0.01 * torch.randn(B, 1, T, generator=g).to(dev))
        runs = {"MSD forward, HIP": lambda: msd(real),
                "MSD forward, ATen": lambda: DO.msd_forward(msd_sd, real),
                "MPD forward, HIP": lambda: mpd(real),
                "MPD forward, ATen": lambda: DO.mpd_forward(mpd_sd, real),
                "feature_matching MSD+MPD, HIP": lambda: pkg.metrics.feature_matching(
                    [msd, mpd], real, fake),
                "feature_matching MSD+MPD, ATen": lambda: aten_fm(real, fake)}
        ms = {k: [] for k in runs}
        with torch.no_grad():
            for step in range(args.warmup + args.steps):
                for name, fn in runs.items():       # alternate: one call of each per round
                    e0 = torch.cuda.Event(enable_timing=True)
                    e1 = torch.cuda.Event(enable_timing=True)
                    t0 = time.monotonic()
                    torch.cuda._sleep(400_000)       # the device is busy while the host enqueues
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    if time.monotonic() - t0 > args.step_limit:
                        sys.exit(f"time_discriminators: '{name}' at {shape} took more than "
                                 f"{args.step_limit} s (step {step})")
                    if step >= args.warmup:
                        ms[name].append(e0.elapsed_time(e1))
        out = {}
        for name, v in ms.items():
            v.sort()
            out[name] = {"median_ms": statistics.median(v), "min_ms": v[0],
                         "p90_ms": v[int(0.9 * (len(v) - 1))]}
            print(f"[{B}, 1, {T}] {name:32s} median {out[name]['median_ms']:9.3f} ms  "
                  f"min {v[0]:9.3f}  p90 {out[name]['p90_ms']:9.3f}", flush=True)
        result[shape] = out
    print(json.dumps({"steps": args.steps, "warmup": args.warmup, "ms": result}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
