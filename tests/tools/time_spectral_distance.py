#!/usr/bin/env python3
"""Time the spectral distances on the README's mel shape, wav [8, 262144] (needs the GPU).

    python tests/tools/time_spectral_distance.py [--batch 8] [--samples 262144] [--calls 50]

The method of time_release_mel.py: everything runs in one process, alternating call by call,
so all variants see the same clocks and the same neighbours.  Each call is bracketed by a HIP
event pair behind a short device-side spin, so the start event, the launches and the end event
are all enqueued while the device is busy and the interval holds the kernels, not the host's
launch path.  5 warm-up calls each, then the timed calls; prints the medians, the spread and
one JSON line.  Timed:

* the fused metrics.mel_distance (release front end) against the unfused form, frontend(wav)
  followed by torch's (m - target).abs().sum((1, 2)), with the front end alone beside them;
* metrics.MultiResolutionSTFT on the same audio: each of the three reference resolutions and
  all three in one call."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--samples", type=int, default=262144)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_spectral_distance: no HIP device (a timing needs the GPU)")
    import __graft_entry__ as ge
    ge.load_package().check_provenance()
    melmod = importlib.import_module(ge.PKG_NAME + ".mel")
    metrics = importlib.import_module(ge.PKG_NAME + ".metrics")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    wav = torch.randn(args.batch, args.samples, generator=g).clamp(-1, 1).to(dev)
    other = (0.9 * wav + 0.01 * torch.randn(wav.shape, generator=g).to(dev)).contiguous()
    front = melmod.ReleaseMelSpectrogram(device=dev)
    target = front(other)
    every = metrics.MultiResolutionSTFT(device=dev)
    singles = [metrics.MultiResolutionSTFT(resolutions=[r], device=dev)
               for r in metrics.REFERENCE_RESOLUTIONS]
    runs = {"release_mel_fft alone": lambda: front(wav),
            "mel_distance fused": lambda: metrics.mel_distance(front, wav, target),
            "mel then torch abs-sum (unfused)": lambda: (front(wav) - target).abs().sum((1, 2))}
    for r, s in zip(metrics.REFERENCE_RESOLUTIONS, singles):
        runs[f"stft_distance {r}"] = (lambda s_=s: s_(wav, other))
    runs["MultiResolutionSTFT (3 resolutions)"] = lambda: every(wav, other)
    for _ in range(args.warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(args.calls):
        for name, fn in runs.items():           # alternate: one call of each per round
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(400_000)           # keeps the device busy while the host enqueues
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    out = {}
    for name, v in ms.items():
        v.sort()
        med = statistics.median(v)
        out[name] = {"median_ms": med, "min_ms": v[0], "p90_ms": v[int(0.9 * (len(v) - 1))]}
        print(f"{name:42s} median {med:.4f} ms  min {v[0]:.4f}  p90 {out[name]['p90_ms']:.4f}")
    fused = out["mel_distance fused"]["median_ms"]
    unfused = out["mel then torch abs-sum (unfused)"]["median_ms"]
    print(f"fused / unfused = {fused / unfused:.3f} (wav [{args.batch}, {args.samples}], "
          f"{args.calls} calls each)")
    print(json.dumps({"shape": [args.batch, args.samples], "calls": args.calls, "ms": out,
                      "fused_over_unfused": fused / unfused}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
