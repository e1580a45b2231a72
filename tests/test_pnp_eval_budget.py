"""Instruction budget of one Levenberg-Marquardt evaluation of the pose solver (CPU: needs hipcc and the LLVM tools beside it only).

The solve is one wave alone on its SIMD and its per-point part runs at the issue floor (profiles/r05_pnp_evaluation_isa.md): an
instruction the compiler adds there is time.  This test reads the diagnostic library's pnp_kernel<float, 1> the way
tools/pnp_eval_isa.py does -- the code between the in-kernel stamps 48 | 49 | 50 | 51 of evaluate_t's mode-2 evaluation, cold blocks
left out -- and holds the pinhole (D = false) instances to what profiles/pose_eval_diet.md reached:

  projection part   at most 2 plain 64-bit zeroing moves (the 28 per-lane sums are assigned, not added to a zeroed register; the
                    zeros of lanes without a point are written in front of the Rodrigues section)
  butterfly part    at most 4 register-to-register 64-bit moves (the lane swaps work on the accumulators where they are)
  whole evaluation  VALU count at most VALU_REACHED + 5 %

Ordinary vector instructions only (v_*): scalar, LDS and memory instructions, waits and branches are not counted."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

VALU_REACHED = 440       # profiles/pose_eval_diet.md, "listing counts": Rodrigues 166 + projection 140 + butterfly 134


@pytest.fixture(scope="module")
def pinhole_instances():
    import pnp_eval_isa as isa
    lib = isa.DBG_LIB
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "accurate_aprilgroup_tracking_amd", "csrc"), "dbg"])
    out = []
    for inst in isa.evaluation_regions(lib):
        parts = {}
        for name, lines in inst.items():
            ops = [isa.parse(l) for l in lines]
            parts[name] = [(re.sub(r"_e(32|64)$", "", o[0]), o[1]) for o in ops if o and o[0].startswith("v_")]
        # the distorted projection divides (1 / (1 + k4 r^2 + ...), correctly rounded: v_div_scale_f64); the pinhole one does not
        if not any(op == "v_div_scale_f64" for op, _ in parts["projection"]):
            out.append(parts)
    assert out, "no pinhole instance of the evaluation found between the stamps"
    return out


def test_projection_part_starts_no_sum_from_a_zeroed_register(pinhole_instances):
    for k, parts in enumerate(pinhole_instances):
        zeroing = [o for o in parts["projection"] if o[0] == "v_mov_b64" and o[1][1] == "0"]
        print("instance %d: projection part %d VALU, %d 64-bit zeroing moves" % (k, len(parts["projection"]), len(zeroing)))
        assert len(zeroing) <= 2


def test_butterfly_part_sums_the_accumulators_in_place(pinhole_instances):
    for k, parts in enumerate(pinhole_instances):
        copies = [o for o in parts["butterfly"] if o[0] == "v_mov_b64" and re.match(r"^v\[\d+:\d+\]$", o[1][1])]
        print("instance %d: butterfly part %d VALU, %d register-to-register 64-bit moves" % (k, len(parts["butterfly"]), len(copies)))
        assert len(copies) <= 4


def test_whole_evaluation_stays_within_its_budget(pinhole_instances):
    for k, parts in enumerate(pinhole_instances):
        n = {name: len(ops) for name, ops in parts.items()}
        total = sum(n.values())
        print("instance %d: %s = %d VALU (reached %d, budget %d)" % (k, n, total, VALU_REACHED, int(VALU_REACHED * 1.05)))
        assert total <= VALU_REACHED * 1.05
