"""Host test of the kernels' LDS layouts (csrc/lds_layout.h): the dynamic-LDS bytes every
launcher requests (``hfg_debug_lds_bytes``) equal tests/golden/lds_index.json, recorded from
the formulas the launchers carried before the layouts were shared with the kernels.

CPU only: the entry point takes no handle and no device.
"""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location(
    "_make_lds_index", os.path.join(HERE, "golden", "make_lds_index.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

with open(M.OUT) as _f:
    INDEX = json.load(_f)
CASES = M.cases()


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


def test_fixture_lists_the_whole_domain():
    """Every family and every case of the domain is in the fixture, and nothing else."""
    assert sorted(INDEX) == sorted(CASES)
    for fam, arglist in CASES.items():
        keys = [M.key(a) for a in arglist]
        assert len(set(keys)) == len(keys)
        assert sorted(INDEX[fam]) == sorted(keys), fam


def test_domain_reaches_every_kernel():
    """The grid is not vacuous: each family has supported cases, the thin kernels exactly the
    channel counts with an instance, and the fp32 conv refuses only oversized windows."""
    for fam, rec in INDEX.items():
        assert any(v > 0 for v in rec.values()), fam
    assert [k for k, v in INDEX["mrf_thin"].items() if v > 0] == ["16", "4", "8"]
    assert [k for k, v in INDEX["mrf_thin_mfma"].items() if v > 0] == ["16"]
    for fam in ("conv_bf16x3", "ups_bf16x3", "resblock_bf16x3", "conv_post", "logmel_fft"):
        assert all(v > 0 for v in INDEX[fam].values()), fam


@pytest.mark.parametrize("family", sorted(CASES))
def test_library_reproduces_the_fixture(lib, family):
    got = {M.key(a): M.record(lib, family, a) for a in CASES[family]}
    bad = {k: (v, INDEX[family][k]) for k, v in got.items() if v != INDEX[family][k]}
    assert not bad, f"{family}: {len(bad)} launches differ (got, fixture): {dict(list(bad.items())[:8])}"


def test_unknown_requests(lib):
    import ctypes
    one = (ctypes.c_int * 1)(16)
    assert lib.hfg_debug_lds_bytes(b"no_such_kernel", one, 1) == -1
    assert lib.hfg_debug_lds_bytes(b"conv_bf16x3", one, 1) == -1   # wrong argument count
    assert M.record(lib, "conv_bf16x3", (0, 3, 1, 0)) == -1        # tile 0 is gone
    assert M.record(lib, "conv_bf16x3", (3, 11, 13, 0)) == -1      # halo 130 > 128
