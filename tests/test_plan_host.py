"""The planner and the packers against tests/golden/plan_index.json, on host-only handles: per
handle the whole ``hfg_debug_plan`` dump (tiles, packings, offsets, whole-ResBlock windows,
halos, splits, thin stages, the sha256 of every packed byte) and the workspace sizes.  The
fixture was recorded from the planner as it stood before the host orchestration was split
into plan / pack / forward units; a difference here is a change of schedule or of packed
bytes, which a refactor must not make (tests/golden/make_plan_index.py)."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN_DIR

_spec = importlib.util.spec_from_file_location("make_plan_index",
                                               os.path.join(GOLDEN_DIR, "make_plan_index.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

with open(os.path.join(GOLDEN_DIR, "plan_index.json")) as _f:
    INDEX = json.load(_f)
CASES = M.cases()


def test_fixture_lists_every_case():
    assert sorted(INDEX) == sorted(name for name, _, _ in CASES)
    assert all(isinstance(INDEX[name]["plan"], dict) for name in M.VERBATIM)


@pytest.mark.parametrize("name,kind,spec", CASES, ids=[c[0] for c in CASES])
def test_plan_matches_fixture(pkg, name, kind, spec):
    got = M.record(pkg, kind, spec)
    want = INDEX[name]
    if isinstance(want["plan"], dict):
        # verbatim dumps: name the first field that moved
        for key in sorted(set(want["plan"]) | set(got["plan"])):
            assert got["plan"].get(key) == want["plan"].get(key), f"{name}: plan[{key!r}] differs"
    assert M.stored(name, got) == want, f"{name}: plan / workspace sizes differ"


def test_plan_commits_and_reports_errors(pkg):
    """hfg_debug_plan commits pending weights first (its error when one is missing) and
    refuses a buffer that is too small."""
    import ctypes
    from oracle import config as C
    h = pkg.Handle(pkg.make_config(**C.V2STAR.kwargs(), precision="f16x3"), -1)
    with pytest.raises(pkg.HfgError) as e:
        h.plan()
    assert e.value.code == -11
    import torch
    for k, v in C.make_state_dict(C.V2STAR, seed=0).items():
        h.set_weight(k, torch.from_numpy(v))
    plan = h.plan()
    assert len(plan["sha256"]) == 64 and plan["packed_len"] > 0
    assert any(L["ew"] != 0 for L in plan["layers"])  # the commit ran: f16x3 exponents set
    small = ctypes.create_string_buffer(16)
    assert h.lib.hfg_debug_plan(h.ptr, small, len(small)) == -22
