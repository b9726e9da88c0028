"""LDS bank model of the full-wave staging writes of ups_bf16x3.hip, on top of
tests/tools/ups_lds_banks.py (which models the 16-B writes of the earlier (quad, half) tasks
and the B-fragment reads; the layout xrow_off and the reads are unchanged).

ds_write_b64 is serviced in 4 groups of 16 contiguous lanes, bank = (a/4) mod 32
(MI355X_MICROARCH.md, LDS): conflict-free iff the 16 lanes cover the 16 8-B slots of 128 B.
The halo write (ds_write2st64_b32, modelled as ds_write_b32: 2 groups of 32 lanes, bank =
(a/4) mod 32) has 16 active lanes.

    python profiles/ups_staging_ab/lds_banks_b64.py
"""
import importlib.util
import os

_p = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests", "tools",
                  "ups_lds_banks.py")
_spec = importlib.util.spec_from_file_location("ups_lds_banks", _p)
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)

WRITE64_GROUPS = [list(range(16 * g, 16 * g + 16)) for g in range(4)]


def extra_cycles(addrs, groups, window, slot):
    """As ups_lds_banks.extra_cycles, for `slot` bytes per lane."""
    tot = 0
    for g in groups:
        slots = {}
        for l in g:
            a = addrs.get(l)
            if a is None:
                continue
            slots.setdefault((a % window) // slot, set()).add(a // slot)
        if slots:
            tot += max(len(v) for v in slots.values()) - 1
    return tot


def simulate_quarters(f, NTILE=256, NW=4):
    """The kernel's staging writes: lane = 4 * (quad of the wave's 16) + 4-channel quarter,
    window quad 1 + 16 wave + (lane >> 2), 8 B at f(row, half) + 8 * (quarter & 1) per frame
    row; and wave 0's halo write: lanes 0-15, channel pair lane & 7 of window row 3 (lanes
    0-7) or NTILE + 4."""
    assert NTILE == 64 * NW
    extra = instr = 0
    for wave in range(NW):
        for j in range(4):
            addrs = {}
            for lane in range(64):
                cq, xq = lane & 3, 1 + wave * 16 + (lane >> 2)
                addrs[lane] = f(4 * xq + j, cq >> 1) + 8 * (cq & 1)
            extra += extra_cycles(addrs, WRITE64_GROUPS, 128, 8)
            instr += 1
    halo = {lane: f(NTILE + 4 if lane & 8 else 3, (lane & 7) >> 2) + 4 * (lane & 3)
            for lane in range(16)}
    h_extra = extra_cycles(halo, [list(range(32)), list(range(32, 64))], 128, 4)
    return extra / instr, h_extra


if __name__ == "__main__":
    w8, hx = simulate_quarters(base.kernel_layout)
    print(f"(quad, quarter) 8-B sub-tasks on all 64 lanes: ds_write_b64 extra/instr {w8:.2f}, "
          f"halo write extra {hx}")
    for cfg, kw in (("cfg 0", dict(WAVES_M=2, WN=4)), ("cfg 1", dict(WAVES_M=1, WN=2))):
        _, r = base.simulate(base.kernel_layout, interleave=True, **kw)
        print(f"B reads, {cfg}: extra/instr {r:.2f}")
