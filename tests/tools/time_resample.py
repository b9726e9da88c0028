#!/usr/bin/env python3
"""Time the ragged multi-channel resampler (csrc/resample.hip) against the route it
replaces and against the fixed-length kernel, with its filter table in both layouts (needs the
GPU).

    python tests/tools/time_resample.py [--batch 8] [--out-samples 262144] [--calls 50]

Workload: `batch` items at 48 kHz -> 22.05 kHz (147 phases, 348 taps), n_samples chosen so that
n_out = --out-samples, ragged device lengths.  Rows:

  (a) the route without the ragged kernel, stereo int16: pcm.to_float on [2 B, n], Resample on
      [2 B, n], torch.mean over the channel pairs.  Three launches, every row full-length: it
      masks nothing and writes no lengths, so it does strictly less than (b) and (c).
  (b) Resample.ragged on [B, 2, n] int16, phase-major table [n_phases][klen] (resample_sinc's).
  (c) the same, tap-major table [klen][n_phases].
  (d) mono float32 [B, n]: Resample.__call__ (resample_sinc, full-length) against
      Resample.ragged with either table.

The protocol of time_pcm.py: everything runs in one process, alternating call by call, so every
row sees the same clocks and the same neighbours.  Each call is bracketed by a HIP event pair
with a short device-side spin queued in front, so the start event, the launches and the end
event are all enqueued while the device is busy and the interval holds the kernels, not the
host's launch path.  5 warm-up calls each, then the timed calls; prints median, min and p90 per
row and one JSON line.  Before timing it checks that (b) and (c) agree bit for bit and that the
mono ragged call with full lengths is bitwise Resample.__call__."""
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

ORIG, NEW = 48000, 22050      # reduced 320 -> 147


def timed(runs, warmup, calls):
    for _ in range(warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(calls):
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
        out[name] = {"median_ms": statistics.median(v), "min_ms": v[0],
                     "p90_ms": v[int(0.9 * (len(v) - 1))]}
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out-samples", type=int, default=262144)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_resample: no HIP device (a timing needs the GPU)")
    import __graft_entry__ as ge
    pkg = ge.load_package()
    if os.environ.get("HFG_ALLOW_OLD_LIB") != "1":   # an A/B against another build's library
        pkg.check_provenance()
    melmod = importlib.import_module(ge.PKG_NAME + ".mel")
    dev = torch.device("cuda:0")
    B = args.batch
    o, w = 320, 147
    n = args.out_samples * o // w
    while -(-w * n // o) < args.out_samples:
        n += 1
    # one handle per table layout (the knob is read when the handle is created)
    pkg.schedule_override("RESAMPLE_TABLE", 0)
    rs_phase = melmod.Resample(ORIG, NEW, device=dev)
    pkg.schedule_override("RESAMPLE_TABLE", 1)
    rs_tap = melmod.Resample(ORIG, NEW, device=dev)
    pkg.schedule_clear("RESAMPLE_TABLE")
    assert rs_tap.out_len(n) == args.out_samples, (n, rs_tap.out_len(n))

    g = torch.Generator().manual_seed(0)
    stereo = (torch.randn(B, 2, n, generator=g).clamp(-1, 1) * 20000).round().to(torch.int16).to(dev)
    mono = stereo[:, 0].to(torch.float32) / 32768.0
    lens_host = [n - 997 * b for b in range(B)]
    lens = torch.tensor(lens_host, dtype=torch.int32, device=dev)
    rows16 = stereo.view(2 * B, n)

    def parent_route():
        f = pkg.pcm.to_float(rows16)
        return rs_tap(f).view(B, 2, -1).mean(dim=1)

    yb, ob = rs_phase.ragged(stereo, lens)
    yc, oc = rs_tap.ragged(stereo, lens)
    assert torch.equal(ob, oc) and torch.equal(yb.view(torch.int32), yc.view(torch.int32)), \
        "the two table layouts disagree"
    for rs in (rs_phase, rs_tap):
        assert torch.equal(rs.ragged(mono)[0].view(torch.int32), rs_tap(mono).view(torch.int32)), \
            "mono ragged is not bitwise Resample.__call__"
    ya = parent_route()
    m = int(ob.min().item()) - 64      # away from every item's end, where (a) sees more input
    print(f"(a) vs (c) inside every length: max |diff| "
          f"{(ya[:, :m] - yc[:, :m]).abs().max().item():.2e}")

    runs = {
        "(a) to_float + Resample + mean, int16 [16, n]": parent_route,
        "(b) ragged int16 [8, 2, n], phase-major": lambda: rs_phase.ragged(stereo, lens),
        "(c) ragged int16 [8, 2, n], tap-major": lambda: rs_tap.ragged(stereo, lens),
        "(d) Resample.__call__ f32 [8, n]": lambda: rs_tap(mono),
        "(d) ragged f32 [8, n], phase-major": lambda: rs_phase.ragged(mono, lens),
        "(d) ragged f32 [8, n], tap-major": lambda: rs_tap.ragged(mono, lens),
    }
    out = timed(runs, args.warmup, args.calls)
    print(f"{ORIG} -> {NEW}, B = {B}, n_samples = {n}, n_out = {args.out_samples}, ragged device "
          f"lengths {lens_host[0]} .. {lens_host[-1]}, {args.calls} calls each")
    for name, r in out.items():
        print(f"{name:48s} median {r['median_ms'] * 1e3:9.1f} us  min {r['min_ms'] * 1e3:9.1f}"
              f"  p90 {r['p90_ms'] * 1e3:9.1f}")
    print(json.dumps({"rates": [ORIG, NEW], "batch": B, "n_samples": n,
                      "n_out": args.out_samples, "calls": args.calls, "rows_ms": out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
