"""Generate tests/golden/schedule_index.json on an MI355X: per case of
tests/test_gpu_schedule.py the launch fingerprint {kernel instance: [launches, flop, bytes]}
of one profiled forward.

Regenerate only with a change that means to move the launch schedule; for a refactor of the
host orchestration, record it from the library of the commit before the change:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_schedule_index.py [OUT.json]
"""
from __future__ import annotations

import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import __graft_entry__ as ge
    import test_gpu_schedule as S
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    index = {name: S.run_case(pkg, spec, dev)[0] for name, spec in S.CASES.items()}
    out = sys.argv[1] if len(sys.argv) > 1 else S.INDEX_PATH
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(index, f, sort_keys=True, indent=0, separators=(",", ":"))
        f.write("\n")
    print(f"{len(index)} cases -> {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
