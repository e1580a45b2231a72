"""Per-call time of overlay.draw_pose (both display lists plus both rasters) against the copy of one 1280 x 720 BGR frame from HBM to
pinned host memory -- the first step of drawing on the host --, measured in one run (profiles/overlay.md).

HIP events on the current stream around calls issued from Python: what a caller pays per call at back-to-back issue, host cost of the
three launches and two allocations included where the device waits for it -- NOT the kernels' own time (for that run this script under
rocprofv3 --kernel-trace --stats, in a run of its own).  "back to back": --calls (1000) calls between two events, median of --blocks
(21) such blocks after 50 warm-up calls; "single": one call between two events, median of 105.  The draw cases and the copy take
turns block by block, so a drift of the box shows in all of them alike.  Prints one JSON line; --out writes it to a file as well.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H = 1280, 720


def tag_points(rng, n, B):
    """n / 4 quads of 40 .. 120 px scattered inside the frame, per batch entry"""
    c = np.stack([rng.uniform(130, W - 130, (B, n // 4)), rng.uniform(130, H - 130, (B, n // 4))], axis=2)
    half = rng.uniform(20, 60, (B, n // 4, 1, 1))
    ang = rng.uniform(0, 2 * np.pi, (B, n // 4, 1)) + np.arange(4) * np.pi / 2
    q = c[:, :, None, :] + half * np.stack([np.cos(ang), np.sin(ang)], axis=3)
    return q.reshape(B, n, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--blocks", type=int, default=21)
    ap.add_argument("--calls", type=int, default=1000)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    from accurate_aprilgroup_tracking_amd import overlay
    rng = np.random.default_rng(0)
    cases = {}
    for name, n, B in (("B=1, 48 points", 48, 1), ("B=16, 48 points", 48, 16), ("B=1, 240 points", 240, 1)):
        frames = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).cuda()
        draw = torch.zeros_like(frames)
        pts = torch.from_numpy(tag_points(rng, n, B)).cuda()
        ok = torch.ones(B, dtype=torch.float64, device="cuda")
        cases[name] = (lambda f=frames, d=draw, p=pts, o=ok: overlay.draw_pose(f, d, p, ok=o))
    src = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda()
    pinned = torch.zeros((H, W, 3), dtype=torch.uint8).pin_memory()
    cases["copy of one frame, HBM to pinned host"] = lambda: pinned.copy_(src, non_blocking=True)

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / calls         # us per call

    for fn in cases.values():
        for _ in range(50):
            fn()
    torch.cuda.synchronize()
    blocks = {k: [] for k in cases}
    singles = {k: [] for k in cases}
    for _ in range(a.blocks):
        for k, fn in cases.items():
            blocks[k].append(timed(fn, a.calls))
    for _ in range(105):
        for k, fn in cases.items():
            singles[k].append(timed(fn, 1))
    result = {"frame": [W, H, 3], "calls_per_block": a.calls, "blocks": a.blocks, "device": torch.cuda.get_device_name(0),
              "cases": {k: {"back_to_back_us": float(np.median(v)), "min_us": float(np.min(v)), "max_us": float(np.max(v)),
                            "single_us": float(np.median(singles[k]))} for k, v in blocks.items()}}
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
