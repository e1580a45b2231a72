"""Instruction budget of one iteration trip of the frame-chained LK body (CPU: needs hipcc and the LLVM tools beside it only).

An LK frame of the fused step is about ten trips of the inner loop of agt_lk_chain_body.h, each executed by four waves that are
alone on their SIMDs: an instruction or a wait inside the trip costs ten times what it costs in the per-frame part
(profiles/lk_trip_bookkeeping.md).  This test reads the level-0 trip of step_kernel<21, 4, 3, true, 1> and of
lk_group_kernel<21, 4, 3, 1> from the product library's listing -- the region is found by rule, tools/isa_mix.py chain_trips /
trip_common_path: the smallest backward-branch region with one barrier, one v_permlane32_swap and the six tap reads, the last of
the kernel's three, the FP64 tie-break block left out -- and holds it to what the bookkeeping change reached:

  VALU count of the trip         at most VALU_REACHED + 5 %
  cross-wave accumulation        at most one LDS add per row leader (lo | hi << 32 as one 64-bit add)
  the wait for the totals        no LDS store between the trip's barrier and the s_waitcnt behind the totals' ds_read_b128
                                 (thread 0 clears the slot of the trip after next once its wave has the totals: the rule of the
                                 slots at iter_sum2)

Before the change the trip had two ds_add_u32 and a ds_write_b128 between the totals' read and its wait, and 99 VALU on this count.
The change did not lower the VALU count: every form with fewer vector instructions (`phase` as a scalar: 92) measured slower on
the card, and the one-test loop condition that measured 0.4 us per frame faster moved four instructions of the back edge from the
scalar to the vector unit (103).  The budget holds the count where the measured optimum left it."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

VALU_REACHED = 103       # profiles/lk_trip_bookkeeping.md, "listing counts"
KERNELS = ["step_kernel<21, 4, 3, true, 1>", "lk_group_kernel<21, 4, 3, 1>"]


@pytest.fixture(scope="module")
def trips():
    import isa_mix as isa
    lib = os.path.join(ROOT, "accurate_aprilgroup_tracking_amd", "libagt_hip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "accurate_aprilgroup_tracking_amd", "csrc"), "all"])
    out = {}
    for name in KERNELS:
        ins = isa.kernel_instructions(name, lib)
        assert ins, "kernel not found: %s" % name
        found = isa.chain_trips(ins)
        assert len(found) == 3, "%s: %d chained trips found, one per level expected" % (name, len(found))
        a, b = found[-1]                                  # levels are unrolled coarse to fine: level 0 comes last
        out[name] = [(op, text) for _, op, text in isa.trip_common_path(ins, a, b)]
    return out


@pytest.mark.parametrize("name", KERNELS)
def test_trip_stays_within_its_valu_budget(trips, name):
    valu = [op for op, _ in trips[name] if op.startswith("v_")]
    print("%s: level-0 trip %d instructions, %d VALU (reached %d, budget %d)" % (name, len(trips[name]), len(valu), VALU_REACHED, int(VALU_REACHED * 1.05)))
    assert len(valu) <= VALU_REACHED * 1.05


@pytest.mark.parametrize("name", KERNELS)
def test_one_lds_add_per_row_leader(trips, name):
    adds = [text for op, text in trips[name] if op.startswith("ds_add")]
    print("%s: %s" % (name, adds))
    assert len(adds) <= 1


@pytest.mark.parametrize("name", KERNELS)
def test_no_lds_store_inside_the_wait_for_the_totals(trips, name):
    ops = [op for op, _ in trips[name]]
    k = ops.index("s_barrier")
    read = next(i for i in range(k + 1, len(ops)) if ops[i] == "ds_read_b128")
    wait = next(i for i in range(read + 1, len(ops)) if ops[i] == "s_waitcnt")
    between = [t for _, t in trips[name][k + 1:wait]]
    print("%s: between the barrier and the totals' wait: %s" % (name, between))
    stores = [t for t in between if t.startswith("ds_") and not t.startswith("ds_read")]
    assert not stores
