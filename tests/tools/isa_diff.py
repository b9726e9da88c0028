#!/usr/bin/env python3
"""Compare the gfx950 device assembly of two source trees, kernel by kernel (CPU only).

    python tests/tools/isa_diff.py OLD_TREE NEW_TREE [--jobs N] [--work DIR]
                                   [--define NAME=VALUE ...]

A refactor of the kernel translation units must leave every kernel's code unchanged
(csrc/resblock_body.h records how little it takes to move the register allocation).  For
each tree this compiles every .hip of its own build.SOURCES to device assembly with its own
build.FLAGS plus ``--cuda-device-only -S``, drops the lines naming ``__hip_cuid_<hash>``
(the compilation unit's id, hashed from the source text), and reports per file and per
kernel symbol whether the text is identical.  For kernels that differ it prints both
sides' register counts, scratch and LDS size from the code-object metadata.

Exit status 0: every file of both trees identical; 1: any difference (a kernel or file on
one side only included); 2: a compile failed.  --work keeps the assembly (<work>/a, <work>/b)
and reuses a file whose source, headers and flags are unchanged.  --define (repeatable) appends
-DNAME=VALUE to both trees' flags, to compare the diagnostic builds of csrc/diag.h as well,
one run each: HFG_ABLATE=1, HFG_CONV_TIMING=1, HFG_RB_TIMING=1.
"""
from __future__ import annotations

import argparse
import glob
import hashlib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

MAX_JOBS = 16
FIGURES = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size",
           ".group_segment_fixed_size")


def load_build(tree: str):
    """The tree's build.py (the package directory is the one that holds build.py + csrc/)."""
    hits = [p for p in glob.glob(os.path.join(tree, "*", "build.py"))
            if os.path.isdir(os.path.join(os.path.dirname(p), "csrc"))]
    if len(hits) != 1:
        sys.exit(f"isa_diff: expected one <package>/build.py with csrc/ in {tree}, found {hits}")
    spec = importlib.util.spec_from_file_location(f"_isa_build_{abs(hash(tree))}", hits[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_asm(build, src: str, out_dir: str):
    """src -> <out_dir>/<src>.s; returns (src, error text or None)."""
    path = os.path.join(build.CSRC, src)
    out = os.path.join(out_dir, src + ".s")
    h = hashlib.sha256(" ".join(build.FLAGS).encode())
    for f in [path] + sorted(glob.glob(os.path.join(build.CSRC, "*.h"))):
        with open(f, "rb") as fh:
            h.update(fh.read() + b"\0")
    key = h.hexdigest()
    if os.path.exists(out) and os.path.exists(out + ".key"):
        with open(out + ".key") as f:
            if f.read().strip() == key:
                return src, None
    cmd = [build.HIPCC, *build.FLAGS, "--cuda-device-only", "-S", path, "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        return src, res.stdout + res.stderr
    with open(out + ".key", "w") as f:
        f.write(key)
    return src, None


def parse(asm_path: str):
    """-> (all lines without the cuid ones, {kernel: its lines}, {kernel: metadata figures})."""
    with open(asm_path) as f:
        lines = [ln.rstrip("\n") for ln in f if "__hip_cuid_" not in ln]
    label = {}
    for i, ln in enumerate(lines):
        m = re.match(r"^([^\s.;:][^\s:]*):", ln)  # "symbol:" (a "; @symbol" comment may follow)
        if m:
            label.setdefault(m.group(1), i)
    kernels, name = {}, None
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            name = m.group(1)
        elif name is not None and ln.strip() == ".end_amdhsa_kernel":
            # the function body (label .. descriptor) holds everything generated for it
            if name not in label:
                sys.exit(f"isa_diff: {asm_path}: no label for kernel {name}")
            kernels[name] = lines[label[name]: i + 1]
            name = None
    meta, cur, inside = {}, None, False
    for ln in lines:
        if ln.strip() == ".amdgpu_metadata":
            inside = True
        elif ln.strip() == ".end_amdgpu_metadata":
            inside = False
        elif inside:
            m = re.match(r"^(  - |    )(\.\w+):\s*(.*)$", ln)
            if not m:
                continue
            if m.group(1) == "  - ":
                cur = {}
            if cur is None:
                continue
            cur[m.group(2)] = m.group(3).strip().strip("'\"")
            if m.group(2) == ".name":
                meta[cur[".name"]] = cur
    return lines, kernels, meta


def figures(meta, k) -> str:
    m = meta.get(k)
    if m is None:
        return "(no metadata)"
    return "  ".join(f"{f.lstrip('.')}={m.get(f, '?')}" for f in FIGURES)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("--jobs", type=int, default=MAX_JOBS)
    ap.add_argument("--work", help="directory that keeps the assembly between runs")
    ap.add_argument("--define", action="append", default=[], metavar="NAME=VALUE",
                    help="append -DNAME=VALUE to both trees' flags (repeatable)")
    args = ap.parse_args()
    jobs = max(1, min(args.jobs, MAX_JOBS))

    tmp = None
    if args.work:
        work = os.path.abspath(args.work)
    else:
        tmp = tempfile.TemporaryDirectory(prefix="isa_diff_")
        work = tmp.name
    sides = []
    for tag, tree in (("a", args.old_tree), ("b", args.new_tree)):
        build = load_build(os.path.abspath(tree))
        build.FLAGS = [*build.FLAGS, *("-D" + d for d in args.define)]
        out_dir = os.path.join(work, tag)
        os.makedirs(out_dir, exist_ok=True)
        sides.append((build, out_dir, [s for s in build.SOURCES if s.endswith(".hip")]))

    tasks = [(b, s, d) for b, d, srcs in sides for s in srcs]
    with ThreadPoolExecutor(jobs) as ex:
        errs = [(d, s, e) for (b, s, d), (_, e) in
                zip(tasks, ex.map(lambda t: compile_asm(t[0], t[1], t[2]), tasks)) if e]
    if errs:
        for d, s, e in errs:
            sys.stderr.write(f"--- {d}/{s}\n{e}\n")
        return 2

    (_, dir_a, srcs_a), (_, dir_b, srcs_b) = sides
    n_files = n_files_same = n_kern = n_kern_same = 0
    for src in sorted(set(srcs_a) | set(srcs_b)):
        n_files += 1
        if src not in srcs_a or src not in srcs_b:
            print(f"{src}: only in the {'old' if src in srcs_a else 'new'} tree")
            continue
        la, ka, ma = parse(os.path.join(dir_a, src + ".s"))
        lb, kb, mb = parse(os.path.join(dir_b, src + ".s"))
        names = sorted(set(ka) | set(kb))
        diff = [k for k in names if ka.get(k) != kb.get(k)]
        n_kern += len(names)
        n_kern_same += len(names) - len(diff)
        same = la == lb
        n_files_same += same
        note = "" if same or diff else "  (the text outside the kernels differs)"
        print(f"{src}: {'identical' if same else 'DIFFERENT'}, "
              f"{len(names) - len(diff)}/{len(names)} kernels identical{note}")
        for k in diff:
            if k not in ka or k not in kb:
                print(f"  {k}: only in the {'old' if k in ka else 'new'} tree")
                continue
            print(f"  {k}: {len(ka[k])} -> {len(kb[k])} lines")
            print(f"    old: {figures(ma, k)}")
            print(f"    new: {figures(mb, k)}")
    ok = n_files_same == n_files
    print(f"isa_diff: {n_files_same}/{n_files} files and {n_kern_same}/{n_kern} kernels "
          f"identical: {'PASS' if ok else 'FAIL'}")
    if tmp:
        tmp.cleanup()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
