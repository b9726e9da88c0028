#!/usr/bin/env python3
"""Time mel.ReleaseMelSpectrogram against the existing mel.MelSpectrogram on the README's
mel shape, wav [8, 262144] (needs the GPU).

    python tests/tools/time_release_mel.py [--batch 8] [--samples 262144] [--calls 50]

Both front ends run in one process, alternating call by call, so they see the same clocks
and the same neighbours; the baseline is the existing kernel in the same run.  Each call is
bracketed by a HIP event pair.  A short device-side spin is queued in front of each pair, so
the start event, the launch and the end event are all enqueued while the device is busy and
the interval holds the kernel, not the host's launch path.  5 warm-up calls each, then the
timed calls; prints the medians, the spread and one JSON line.  Also timed: the ragged call
(device lengths, frame counts written)."""
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
        sys.exit("time_release_mel: no HIP device (a timing needs the GPU)")
    import __graft_entry__ as ge
    if os.environ.get("HFG_ALLOW_OLD_LIB") != "1":   # an A/B against another build's library
        ge.load_package().check_provenance()
    melmod = importlib.import_module(ge.PKG_NAME + ".mel")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    wav = torch.randn(args.batch, args.samples, generator=g).clamp(-1, 1).to(dev)
    lens = torch.tensor([args.samples - 997 * b for b in range(args.batch)], dtype=torch.int32,
                        device=dev)
    old, new = melmod.MelSpectrogram(device=dev), melmod.ReleaseMelSpectrogram(device=dev)
    runs = {"MelSpectrogram (logmel_fft)": lambda: old(wav),
            "ReleaseMelSpectrogram (release_mel_fft)": lambda: new(wav),
            "ReleaseMelSpectrogram, device lengths": lambda: new(wav, lens)}
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
        print(f"{name:45s} median {med:.4f} ms  min {v[0]:.4f}  p90 {out[name]['p90_ms']:.4f}")
    a, b = (out[k]["median_ms"] for k in list(runs)[:2])
    print(f"release / existing = {b / a:.3f} (wav [{args.batch}, {args.samples}], "
          f"{args.calls} calls each)")
    print(json.dumps({"shape": [args.batch, args.samples], "calls": args.calls, "ms": out,
                      "release_over_existing": b / a}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
