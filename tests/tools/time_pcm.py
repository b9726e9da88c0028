#!/usr/bin/env python3
"""Time the four PCM-boundary launches (csrc/pcm.hip) and glue.resynthesize_pcm against
glue.resynthesize on the README's mel shape, pcm [8, 262144] (needs the GPU).

    python tests/tools/time_pcm.py [--batch 8] [--samples 262144] [--calls 50]

The protocol of time_release_mel.py: everything runs in one process, alternating call by call,
so every row sees the same clocks and the same neighbours.  Each call is bracketed by a HIP
event pair with a short device-side spin queued in front, so the start event, the launch and
the end event are all enqueued while the device is busy and the interval holds the kernel, not
the host's launch path.  5 warm-up calls each, then the timed calls; prints median, min and p90
per row, each kernel's achieved bytes/s (the bytes its definition moves, from the shapes)
beside the 8 TB/s datasheet figure, and one JSON line.  release_mel_fft is timed in the same
rounds: the front end's own launch is the yardstick for "launch-bound microsecond kernels".
The launches go through the C ABI on preallocated buffers (ragged device lengths); the two
chains through the Python layer."""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_DATASHEET = 8.0e12   # bytes/s


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
    ap.add_argument("--samples", type=int, default=262144)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_pcm: no HIP device (a timing needs the GPU)")
    import __graft_entry__ as ge
    pkg = ge.load_package()
    pkg.check_provenance()
    lib = pkg.load_library()
    glue = importlib.import_module(ge.PKG_NAME + ".glue")
    ck = importlib.import_module(ge.PKG_NAME + ".checkpoint")
    S = importlib.import_module(ge.PKG_NAME + ".synth")
    melmod = importlib.import_module(ge.PKG_NAME + ".mel")
    dev = torch.device("cuda:0")
    B, N = args.batch, args.samples
    g = torch.Generator().manual_seed(0)
    pcm = (torch.randn(B, N, generator=g).clamp(-1, 1) * 20000).round().to(torch.int16).to(dev)
    lens_host = [N - 997 * b for b in range(B)]
    lens = torch.tensor(lens_host, dtype=torch.int32, device=dev)
    peak = torch.empty(B, dtype=torch.float32, device=dev)
    wav = torch.empty(B, N, dtype=torch.float32, device=dev)
    q = torch.empty(B, N, dtype=torch.int16, device=dev)
    offsets = torch.empty(B + 1, dtype=torch.int64, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def ok(rc):
        if rc != 0:
            sys.exit(f"time_pcm: {lib.hfg_mel_last_error().decode()}")

    front = melmod.ReleaseMelSpectrogram(device=dev)
    launches = {
        "pcm_peak<int16> (+ memset)": lambda: ok(lib.hfg_pcm_peak(p(pcm), 0, B, N, p(lens), p(peak), st)),
        "pcm_to_float<int16> plain": lambda: ok(lib.hfg_pcm_to_float(p(pcm), 0, B, N, p(lens), None,
                                                                    0.95, p(wav), st)),
        "pcm_to_float<int16> normalised": lambda: ok(lib.hfg_pcm_to_float(p(pcm), 0, B, N, p(lens),
                                                                         p(peak), 0.95, p(wav), st)),
        "pcm_offsets": lambda: ok(lib.hfg_pcm_offsets(p(lens), B, N, p(offsets), st)),
        "pcm_from_float padded": lambda: ok(lib.hfg_pcm_from_float(p(wav), B, N, p(lens), 0, None,
                                                                  p(q), st)),
        "pcm_from_float packed": lambda: ok(lib.hfg_pcm_from_float(p(wav), B, N, p(lens), 0,
                                                                  p(offsets), p(q), st)),
        "release_mel_fft (device lengths)": lambda: front(wav, lens),
    }
    valid = sum(lens_host)
    moved = {   # bytes each kernel's definition moves
        "pcm_peak<int16> (+ memset)": 2 * valid,
        "pcm_to_float<int16> plain": 2 * valid + 4 * B * N,
        "pcm_to_float<int16> normalised": 2 * valid + 4 * B * N,
        "pcm_from_float padded": 4 * valid + 2 * B * N,
        "pcm_from_float packed": 6 * valid,
    }
    out = timed(launches, args.warmup, args.calls)
    print(f"pcm [{B}, {N}] int16, ragged device lengths, {args.calls} calls each")
    for name, r in out.items():
        line = (f"{name:34s} median {r['median_ms'] * 1e3:8.1f} us  min {r['min_ms'] * 1e3:8.1f}"
                f"  p90 {r['p90_ms'] * 1e3:8.1f}")
        if name in moved:
            r["bytes"] = moved[name]
            r["bytes_per_s"] = moved[name] / (r["median_ms"] * 1e-3)
            line += (f"  {r['bytes_per_s'] / 1e12:5.2f} TB/s "
                     f"({r['bytes_per_s'] / HBM_DATASHEET:.0%} of the 8 TB/s datasheet figure)")
        print(line)

    gen = ck.generator_from_release_config(
        {"resblock": "1", "upsample_rates": [8, 8, 2, 2], "upsample_kernel_sizes": [16, 16, 4, 4],
         "upsample_initial_channel": 512, "resblock_kernel_sizes": [3, 7, 11],
         "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5], [1, 3, 5]]}).eval()
    gen.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v))
                         for k, v in S.random_state_dict(S.V1, seed=5).items()})
    gen = gen.to(dev)
    audio = pkg.pcm.to_float(pcm, lens, normalize=True)
    chains = {
        "resynthesize (float in, float out)": lambda: glue.resynthesize(gen, front, audio, lens),
        "resynthesize_pcm (int16 in, int16 out)": lambda: glue.resynthesize_pcm(
            gen, front, pcm, lens, normalize=True),
    }
    cout = timed(chains, args.warmup, args.calls)
    for name, r in cout.items():
        print(f"{name:40s} median {r['median_ms']:9.4f} ms  min {r['min_ms']:9.4f}"
              f"  p90 {r['p90_ms']:9.4f}")
    a, b = (cout[k]["median_ms"] for k in chains)
    print(f"resynthesize_pcm - resynthesize = {(b - a) * 1e3:.1f} us ({b / a:.4f} x)")
    print(json.dumps({"shape": [B, N], "calls": args.calls, "launches_ms": out, "chains_ms": cout,
                      "pcm_over_float_chain": b / a}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
