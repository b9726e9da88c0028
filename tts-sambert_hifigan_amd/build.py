"""Build libhifigan_hip.so in-tree with hipcc for gfx950 (no torch, no JIT cache).

    python tts-sambert_hifigan_amd/build.py          # or __graft_entry__.build()
"""
from __future__ import annotations

import hashlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG_DIR, "csrc")
LIB_NAME = "libhifigan_hip.so"
LIB_PATH = os.path.join(PKG_DIR, LIB_NAME)
SOURCES = ["conv_kernels.hip", "conv_bf16x3.hip", "resblock_bf16x3.hip",
           "mrf_thin.hip", "mrf_thin_mfma.hip", "ups_bf16x3.hip", "probe.hip", "hifigan_capi.cpp",
           "plan.cpp", "pack.cpp", "forward.cpp", "inspect_capi.cpp", "mel_kernels.hip",
           "resample.hip", "pcm.hip", "spectral_distance.hip", "mel_capi.cpp", "relmel_capi.cpp",
           "resample_capi.cpp", "pcm_capi.cpp", "specdist_capi.cpp", "disc_conv.hip",
           "disc_thin.hip", "disc_capi.cpp"]

OBJ_DIR = os.path.join(PKG_DIR, "build")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = [
    "--offload-arch=gfx950",
    # code object v5: loadable by both /opt/rocm (7.2) and torch's bundled HIP runtime
    "-mcode-object-version=5",
    "-O3", "-std=c++17", "-fPIC",
    # no SLP packing of scalar f32 ops into v_pk_add/mul_f32 (each costs ~20 extra cycles
    # beside MFMAs, MI355X_MICROARCH.md; same-box A/B +0.3-0.5 %, profiles/r04/ab/nslp)
    "-fno-slp-vectorize",
    "-Wall", "-Wno-unused-result",
] + os.environ.get("HFG_EXTRA_FLAGS", "").split()  # A/B variants (profiles/r04/ab.sh)


def _tree_files():
    """Every file the library is built from: csrc/* (sources and headers) and include/*.h."""
    inc = os.path.join(PKG_DIR, "..", "include")
    files = [os.path.join(CSRC, f) for f in os.listdir(CSRC)
             if f.endswith((".hip", ".cpp", ".h"))]
    files += [os.path.join(inc, f) for f in os.listdir(inc) if f.endswith(".h")]
    return sorted(files, key=os.path.basename)


def source_hash() -> str:
    """16 hex digits of sha256 over the build inputs (file names + contents of csrc/ and
    include/, the compiler flags).  Embedded in the library (``hfg_version``) so a loaded
    binary can be matched to the tree it claims to come from."""
    h = hashlib.sha256()
    for f in _tree_files():
        h.update(os.path.basename(f).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
        h.update(b"\0")
    h.update(" ".join(FLAGS).encode())
    return h.hexdigest()[:16]


def _obj_key(src: str, tree: str) -> str:
    """What an object depends on: its source, every header, the flags (and, for the C ABI
    unit that embeds it, the tree hash)."""
    h = hashlib.sha256()
    for f in [os.path.join(CSRC, src)] + [f for f in _tree_files() if f.endswith(".h")]:
        with open(f, "rb") as fh:
            h.update(fh.read())
    h.update(" ".join(FLAGS).encode())
    if src == "hifigan_capi.cpp":
        h.update(tree.encode())
    return h.hexdigest()


def _stale(tree: str) -> bool:
    stamp = os.path.join(OBJ_DIR, "lib.stamp")
    if not os.path.exists(LIB_PATH) or not os.path.exists(stamp):
        return True
    with open(stamp) as f:
        return f.read().strip() != tree


def _obj(src: str) -> str:
    return os.path.join(OBJ_DIR, os.path.splitext(src)[0] + ".o")


def _compile(src: str, verbose: bool, tree: str):
    extra = [f'-DHFG_SRC_HASH="{tree}"'] if src == "hifigan_capi.cpp" else []
    cmd = [HIPCC, *FLAGS, *extra, "-c", os.path.join(CSRC, src), "-o", _obj(src) + ".tmp"]
    if verbose:
        print("[build]", " ".join(cmd), flush=True)
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        return src, res.stdout + res.stderr
    os.replace(_obj(src) + ".tmp", _obj(src))
    with open(_obj(src) + ".key", "w") as f:
        f.write(_obj_key(src, tree))
    return src, None


def build(force: bool = False, verbose: bool = True) -> str:
    """Compile the HIP kernels + C ABI into ``libhifigan_hip.so`` next to this file: one
    object per source (in parallel, only those whose inputs' CONTENT changed — not
    mtimes, which a copied tree does not preserve), then one link.  The tree hash is
    compiled into ``hfg_version`` and written to ``build/lib.stamp``."""
    tree = source_hash()
    if not force and not _stale(tree):
        return LIB_PATH
    os.makedirs(OBJ_DIR, exist_ok=True)

    def obj_stale(src):
        if force or not os.path.exists(_obj(src)) or not os.path.exists(_obj(src) + ".key"):
            return True
        with open(_obj(src) + ".key") as f:
            return f.read().strip() != _obj_key(src, tree)

    todo = [src for src in SOURCES if obj_stale(src)]
    jobs = max(1, min(len(todo), int(os.environ.get("MAX_JOBS", "8"))))
    with ThreadPoolExecutor(jobs) as ex:
        errs = [(src, err) for src, err in ex.map(lambda s_: _compile(s_, verbose, tree), todo)
                if err]
    if errs:
        for src, err in errs:
            sys.stderr.write(f"--- {src}\n{err}")
        raise RuntimeError(f"hipcc failed on {', '.join(s_ for s_, _ in errs)}")
    tmp = LIB_PATH + ".tmp"
    cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC",
           *[_obj(src) for src in SOURCES], "-o", tmp]
    if verbose:
        print("[build]", " ".join(cmd), flush=True)
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        sys.stderr.write(res.stdout + res.stderr)
        raise RuntimeError(f"hipcc link failed with exit code {res.returncode}")
    os.replace(tmp, LIB_PATH)
    with open(os.path.join(OBJ_DIR, "lib.stamp"), "w") as f:
        f.write(tree)
    return LIB_PATH


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
