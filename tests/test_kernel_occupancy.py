"""Register bounds that an occupancy claim of DESIGN.md rests on and that tests/test_kernel_resources.py does not hold (CPU only:
the figures come from the built library's code-object notes).

lk_group_kernel<21, 4, 6, 1> -- the chained LK role's group launch at six pyramid levels -- is a 256-thread workgroup, one wave per
SIMD: at up to 256 registers of the 512-register file two workgroups share a CU, at 257 it is one.  The kernel stands at exactly 256
since the iteration loop of agt_lk_chain_body.h became two loops (profiles/pose_handover.md), so the next register an edit of that body
costs would halve its occupancy without any other test noticing."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "accurate_aprilgroup_tracking_amd", "libagt_hip.so")


@pytest.fixture(scope="module")
def rows():
    import kernel_resources
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    return kernel_resources.kernel_rows(LIB)


def test_six_level_lk_group_kernel_keeps_two_workgroups_per_cu(rows):
    k = [r for r in rows if "lk_group_kernel<21, 4, 6, 1>" in r["name"]]
    assert len(k) == 1, [r["name"] for r in k]
    assert k[0]["vgpr"] <= 256 and k[0]["vspill"] == 0 and k[0]["scratch"] == 0, k[0]
