"""Generate tests/golden/lds_index.json: the dynamic-LDS bytes every kernel launcher requests
(``hfg_debug_lds_bytes``) over the shapes its kernel family accepts.

The fixture pins the host side of each kernel's LDS layout (csrc/lds_layout.h), so a refactor
of the layouts can be checked on the CPU; the device side is pinned by tests/tools/isa_diff.py.
Regenerate it only with a change that means to move a layout, and for a refactor from the
library of the commit BEFORE the change (plus this entry point):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_lds_index.py

``tests/test_lds_layout_host.py`` imports ``cases`` / ``record`` from here and asserts equality.
A value of -1 records that the family has no kernel for those arguments.
"""
from __future__ import annotations

import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(HERE, "lds_index.json")
MAX_DIL, BF16X3_MAX_HALO = 16, 128


def bf16x3_supported(kt, dil):
    return 1 <= dil <= MAX_DIL and 1 <= kt <= 16 and (kt - 1) * dil <= BF16X3_MAX_HALO


def cases():
    """{family: [argument tuples]}, the argument order of hfg_debug_lds_bytes."""
    taps_dils = [(kt, d) for kt in range(1, 17) for d in range(1, MAX_DIL + 1)]
    return {
        # (tile, taps, dilation, LDS-staged epilogue)
        "conv_bf16x3": [(t, kt, d, e) for t in range(1, 7) for kt, d in taps_dils
                        if bf16x3_supported(kt, d) for e in (0, 1)],
        "ups_bf16x3": [(c,) for c in (0, 1)],
        # (channels, window columns, convs of the launch)
        "resblock_bf16x3": [(c, w, n) for c in (32, 64, 128) for w in (256, 512)
                            for n in range(1, 17)],
        # every channel count: -1 where the family has no kernel for it
        "mrf_thin": [(c,) for c in range(1, 65)],
        "mrf_thin_mfma": [(c,) for c in range(1, 65)],
        # (tile, taps, dilation): -1 where fp32_conv_supported refuses
        "conv1d_mfma_f32": [(t, kt, d) for t in range(3) for kt, d in taps_dils],
        "conv_post": [(c,) for c in (16, 32, 64, 128, 512)],
        # (n_fft, hop, n_mels, frames per wave)
        "logmel_fft": [(n, h, m, f) for n in (1 << s for s in range(4, 13))
                       for h in (n // 4, n // 2) for m in (13, 80, 128) for f in (1, 2)],
    }


def key(args) -> str:
    return ",".join(str(a) for a in args)


def record(lib, family, args) -> int:
    arr = (ctypes.c_int * len(args))(*args)
    return int(lib.hfg_debug_lds_bytes(family.encode(), arr, len(args)))


def main():
    import __graft_entry__ as ge
    lib = ge.load_package().load_library()
    index = {fam: {key(a): record(lib, fam, a) for a in arglist}
             for fam, arglist in cases().items()}
    with open(OUT, "w") as f:
        json.dump(index, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    n = sum(len(v) for v in index.values())
    print(f"{n} launches -> {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
