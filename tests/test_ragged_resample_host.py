"""hfg_resample_ragged / mel.Resample.ragged on the CPU: the header and its binding, every
argument refusal (they come before any HIP call, so a host-only handle and host buffers do),
the output-length formula, the properties the case table of ragged_resample_cases.py claims
(recomputed), the room the bar leaves a correct kernel (its arithmetic emulated in numpy) and
four mutants of the reference that the GPU test must be able to see."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

import mel_cases as MC
import ragged_resample_cases as RC
from conftest import ROOT

NEW_SYMBOLS = {"hfg_resample_ragged"}
ALL_PAIRS = RC.PAIRS + [RC.IDENTITY]
ALL_IDS = RC.PAIR_IDS + ["22050-22050"]


def _host_handle(lib, orig, new):
    h = ctypes.c_void_p()
    assert lib.hfg_resample_create(orig, new, 6, 0.99, -1, ctypes.byref(h)) == 0
    return h


def test_header_and_signatures_in_sync(pkg):
    """include/hifigan_hip_resample.h declares exactly the new entry, exported and bound with
    the listed argtypes, and hifigan_hip.h includes it."""
    lib = pkg.load_library()
    src = open(os.path.join(ROOT, "include", "hifigan_hip_resample.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    syms = set(re.findall(r"\b(hfg_[a-z0-9_]+)\s*\(", src))
    assert syms == NEW_SYMBOLS == set(pkg._lib.RESAMPLE_EX_SIGNATURES)
    for s in syms:
        assert hasattr(lib, s), f"missing export {s}"
        res, args = pkg._lib.RESAMPLE_EX_SIGNATURES[s]
        assert getattr(lib, s).argtypes == args and getattr(lib, s).restype == res
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    assert pkg._lib.RESAMPLE_EX_SIGNATURES["hfg_resample_ragged"] == (
        ctypes.c_int, [vp, vp, ctypes.c_int, i64, i64, i64, vp, vp, vp, vp])
    assert '#include "hifigan_hip_resample.h"' in open(os.path.join(ROOT, "include",
                                                                   "hifigan_hip.h")).read()
    assert re.search(r"\bHFG_RESAMPLE_MAX_CHANNELS\s*=\s*8\b", src)
    assert pkg._lib.RESAMPLE_MAX_CHANNELS == 8
    assert "RESAMPLE_TABLE" in pkg._lib.schedule_knobs()


def test_every_refusal_is_einval_and_writes_nothing(pkg):
    """Every HFG_EINVAL of the header on a host-only handle: the arguments first, the handle
    last.  x, y and out_lengths are host buffers filled with a guard value; none moves."""
    lib = pkg.load_library()
    h = _host_handle(lib, 24000, 22050)
    n = 64
    x = np.full(8 * n, 12345, np.int16)
    y = np.full(8 * n, -7.5, np.float32)
    ol = np.full(4, -99, np.int32)
    lens = np.full(4, n, np.int32)
    px, py, pol, pl = (a.ctypes.data_as(ctypes.c_void_p) for a in (x, y, ol, lens))

    def refused(rc, word):
        assert rc == -22
        msg = lib.hfg_mel_last_error()
        assert msg and word in msg, (word, msg)
        assert (x == 12345).all() and (y == -7.5).all() and (ol == -99).all() and (lens == n).all()

    call = lib.hfg_resample_ragged
    refused(call(None, px, 0, 1, 1, n, pl, py, pol, None), b"NULL")
    refused(call(h, None, 0, 1, 1, n, pl, py, pol, None), b"NULL")
    refused(call(h, px, 0, 1, 1, n, pl, None, pol, None), b"NULL")
    for B in (0, -1, 65536):
        refused(call(h, px, 0, B, 1, n, pl, py, pol, None), b"B must")
    for C in (0, -2, 9, 1 << 40):
        refused(call(h, px, 0, 1, C, n, pl, py, pol, None), b"C must")
    for bad_n in (0, -4):
        refused(call(h, px, 0, 1, 1, bad_n, pl, py, pol, None), b"n_samples")
    for dtype in (-1, 2, 7):
        refused(call(h, px, dtype, 1, 1, n, pl, py, pol, None), b"dtype")
    refused(call(h, px, 0, 1, 1, 2 ** 31, pl, py, pol, None), b"INT32_MAX")
    up = _host_handle(lib, 11025, 22050)            # n fits, n_out = 2 n does not
    refused(call(up, px, 0, 1, 1, 2 ** 30 + 1, pl, py, pol, None), b"INT32_MAX")
    # 44100 -> 8000: a block's input span is 4 * 441 + 509 = 2273 floats a channel, so 8 channels
    # (72736 B) do not fit the 64 KiB tile and 7 (63644 B) do
    wide = _host_handle(lib, 44100, 8000)
    refused(call(wide, px, 0, 1, 8, n, pl, py, pol, None), b"LDS")
    refused(call(wide, px, 0, 1, 7, n, pl, py, pol, None), b"host-only")
    # valid arguments, NULL lengths and out_lengths included: only the handle is in the way
    refused(call(h, px, 0, 4, 2, n, pl, py, pol, None), b"host-only")
    refused(call(h, px, 1, 1, 8, n, None, py, None, None), b"host-only")
    for hh in (h, up, wide):
        lib.hfg_resample_destroy(hh)


def test_python_layer_refuses_cpu_tensors(pkg):
    """No CPU fallback: a CPU tensor raises before anything else is looked at (no handle can
    be created without a device, so the method is called unbound)."""
    melmod = importlib.import_module("tts_sambert_hifigan_amd.mel")
    with pytest.raises(RuntimeError, match="HIP tensor"):
        melmod.Resample.ragged(object(), torch.zeros(2, 16, dtype=torch.int16))
    with pytest.raises(RuntimeError, match="HIP tensor"):
        melmod.Resample.ragged(object(), torch.zeros(2, 2, 16), [16, 3])


@pytest.mark.parametrize("orig,new", ALL_PAIRS, ids=ALL_IDS)
def test_out_len_and_case_table(pkg, orig, new):
    """hfg_resample_out_len is mel_cases.out_len on every case length and on 0 (equal rates
    included: the handle is creatable), and the case table has the properties its docstring
    claims."""
    lib = pkg.load_library()
    h = _host_handle(lib, orig, new)
    batches = RC.batches(orig, new)
    N = RC.n_samples(orig, new)
    n_out = MC.out_len(orig, new, N)
    for n in {0, N} | {n for b in batches for n in b}:
        assert lib.hfg_resample_out_len(h, n) == MC.out_len(orig, new, n), n
    lib.hfg_resample_destroy(h)
    assert MC.out_len(orig, new, 0) == 0
    assert RC.signal(orig, new).shape == (3, 8, N) and RC.signal_s16(orig, new).dtype == np.int16
    assert all(len(b) == 3 and b[0] == N for b in batches)
    if (orig, new) == RC.IDENTITY:
        assert n_out == N and {b[1] for b in batches} == {255, 256, 257}
        assert {b[2] for b in batches} == {0, 1, 2}
        return
    ls = MC.resample_lengths(orig, new)
    w = MC.width_of(orig, new)
    assert N == max(ls) <= 2230 and RC.blocks(n_out) >= 2
    hit = MC.out_hit(orig, new)
    assert hit == MC.OUT_HIT[(orig, new)]
    edges = [MC.out_len(orig, new, b[1]) for b in batches]
    assert all(b[1] in ls for b in batches)
    assert all(e in hit and e < n_out for e in edges)
    assert set(edges) == {t for t in hit if t < n_out}          # every reachable edge is used
    assert sorted(b[2] for b in batches) == sorted([0, 1, 2, w, w + 1])
    # some item ends inside a block (a straddled block) with one or more whole blocks past it
    assert any(MC.out_len(orig, new, n) % 256 and
               RC.blocks(n_out) > RC.blocks(MC.out_len(orig, new, n))
               for b in batches for n in b[1:])
    # ... and an empty item: every block of it lies past its end
    assert any(b[2] == 0 for b in batches)


@pytest.mark.parametrize("orig,new", ALL_PAIRS, ids=ALL_IDS)
def test_kernel_arithmetic_under_the_bar(orig, new, evidence):
    """The kernel's arithmetic on the CPU (mel_cases.fma_chain per channel on the cropped item,
    then the fp32 channel sum and division) stays within RESAMPLE_BAR x max|x| of ragged_ref on
    every case and channel count, int16 input included: the bar has room for a correct kernel."""
    x = RC.signal(orig, new)
    xs = RC.signal_s16(orig, new).astype(np.float32) / np.float32(32768)
    scale = float(np.abs(x).max())
    worst = 0.0
    for lens in RC.batches(orig, new):
        for C in RC.CHANNELS:
            for src in (x, xs):
                got = RC.chain_ref(src[:, :C], lens, orig, new).astype(np.float64)
                ref = RC.ragged_ref(src[:, :C], lens, orig, new)
                assert got.shape == ref.shape
                worst = max(worst, float(np.abs(got - ref).max()) / scale)
    evidence(f"ragged resample {orig}->{new}: fp32 chains + channel mean vs float64 reference "
             f"{worst:.2e} x max|x| (bar {MC.RESAMPLE_BAR:g})")
    assert worst <= MC.RESAMPLE_BAR


@pytest.mark.parametrize("mutant", list(RC.MUTANTS))
def test_reference_mutants_leave_the_bar(mutant, evidence):
    """Each mutant of ragged_ref (one sample past the length read; channel 0 only; the sum
    divided by C - 1; the batch's n_samples as every item's length) moves one or more listed
    cases of EVERY pair by more than the bar, so the GPU test can see that fault."""
    seen = []
    # the identity filter has one tap: a sample past the length reaches no output inside it
    pairs = RC.PAIRS if mutant == "one_sample_past_the_length" else ALL_PAIRS
    for (orig, new) in pairs:
        x = RC.signal(orig, new)
        scale = float(np.abs(x).max())
        caught = 0
        for lens in RC.batches(orig, new):
            for C in RC.CHANNELS:
                if C == 1 and mutant in ("channel_0_only", "divided_by_C_minus_1"):
                    continue
                ref = RC.ragged_ref(x[:, :C], lens, orig, new)
                mut = RC.ragged_ref(x[:, :C], lens, orig, new, **RC.MUTANTS[mutant])
                caught += float(np.abs(mut - ref).max()) > MC.RESAMPLE_BAR * scale
        assert caught, (mutant, orig, new)
        seen.append(f"{orig}->{new} {caught}")
    evidence(f"ragged mutant {mutant}: cases that catch it: " + ", ".join(seen))
