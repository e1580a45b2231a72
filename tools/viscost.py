#!/usr/bin/env python3
"""Cost of the visibility rule of the reproject refresh (agt_tracker_visibility): one reproject-mode frame (pyramid -> LK -> PnP +
refresh, stage by stage in stream order) with the rule off and on, on the closed bodies of tests/visibility_scenes.py (640x480; 12 tags =
48 corners, the one-wave solve; 24 tags = 96 corners, the cooperating-wave solve), one stream.  HIP events around `--steps` steps after a
warm-up, the tracker re-seeded (detector-fed frame 0) before every block, median of `--blocks` blocks; off and on alternate block by
block.  The frames are walked back and forth so that every step is a one-frame motion.

--package-root DIR times another checkout of the project (its accurate_aprilgroup_tracking_amd with a built library; the parent commit,
say) on the same scenes: a build without the rule reports the off column only.

    python tools/viscost.py [--steps 200] [--blocks 9] [--package-root DIR] [--label NAME]        (one table per run, on stdout)
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--label", default="this tree")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)                                          # (the oracle behind the scenes' Rodrigues)
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch
    from oracle import cvoracle
    cvoracle.build()
    import visibility_scenes as S
    from accurate_aprilgroup_tracking_amd import hiplib as H
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    assert torch.cuda.is_available(), "needs a GPU"
    assert os.path.abspath(H.LIB_PATH).startswith(os.path.abspath(args.package_root)), H.LIB_PATH
    print("# %s: corners  view_deg  us_per_frame_off  us_per_frame_on  extra_us  accepted_on  visible_tags_on   (640x480, reproject, 1 stream, "
          "%d steps per block, median of %d blocks)" % (args.label, args.steps, args.blocks))
    for T in (12, 24):
        clip = S.ClosedBodyClip.get(T)
        F, deg = len(clip), S.VIEW_DEG[T]
        walk = list(range(1, F)) + list(range(F - 2, -1, -1))
        frames = [torch.from_numpy(clip.frame(k)[None]).cuda().contiguous() for k in range(F)]
        c0 = torch.from_numpy(clip.corners(0)[None]).cuda().contiguous()
        m0 = torch.from_numpy(clip.seed_mask(deg)[None]).cuda().contiguous()
        trk = StreamTracker(clip.width, clip.height, clip.obj, clip.K, None, n_streams=1, reproject=True)
        has_rule = hasattr(trk, "visibility")
        so = trk.new_state_buffer(args.warmup + args.steps)
        times = {False: [], True: []}
        acc = vis = 0
        for blk in range(2 * args.blocks):
            on = bool(blk & 1)
            if on and not has_rule:
                continue
            if has_rule:
                trk.visibility(deg if on else 0.0)
            trk.reset()
            trk.step_detected(frames[0], c0, m0)
            for i in range(args.warmup):
                trk.step(frames[walk[i % len(walk)]], so[i])
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(args.warmup, args.warmup + args.steps):
                trk.step(frames[walk[i % len(walk)]], so[i])
            e1.record()
            torch.cuda.synchronize()
            times[on].append(e0.elapsed_time(e1) * 1e3 / args.steps)
            if on:
                r = so.cpu().numpy()[args.warmup:, 0]
                acc, vis = int(r[:, H.ST_OK].sum()), float(r[:, H.ST_NVISIBLE].mean())
        off = float(np.median(times[False]))
        if has_rule:
            onv = float(np.median(times[True]))
            print("%4d %6g %12.2f %12.2f %9.2f %6d/%d %8.2f" % (4 * T, deg, off, onv, onv - off, acc, args.steps, vis), flush=True)
        else:
            print("%4d %6s %12.2f %12s %9s" % (4 * T, "-", off, "-", "-"), flush=True)
        del trk, frames


if __name__ == "__main__":
    main()
