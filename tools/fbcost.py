#!/usr/bin/env python3
"""Cost of the tracker's forward-backward check (agt_tracker_fb_check): the serial step (pipeline depth 0: pyramid -> LK [-> backward
LK] -> PnP in stream order) per frame with the check off and on, c2 geometry (1280x720, 48 corners), 1 and 64 streams.  HIP events
around `--steps` steps after a warm-up, the tracker re-seeded before every block, median of `--blocks` blocks; off and on alternate
block by block.  Every stream sees the same rendered frames, walked back and forth so that every step is a one-frame motion.

    python tools/fbcost.py [--streams 1,64] [--steps 210] [--blocks 15] > profiles/fb_check_cost.txt
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,64")
    ap.add_argument("--steps", type=int, default=210)
    ap.add_argument("--warmup", type=int, default=14)
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--fb-px", type=float, default=1.0)
    ap.add_argument("--render-frames", type=int, default=8)
    args = ap.parse_args()
    import torch
    from accurate_aprilgroup_tracking_amd import hiplib as H
    from accurate_aprilgroup_tracking_amd import synthetic as syn
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    assert torch.cuda.is_available(), "needs a GPU"
    assert args.steps >= 200, "at least 200 steps per block"
    F = args.render_frames
    seq = syn.Sequence(1280, 720, n_tags=12, n_frames=F, seed=1, supersample=2)
    walk = list(range(1, F)) + list(range(F - 2, -1, -1))           # 1 .. F-1, F-2 .. 0: back at frame 0 after 2 (F - 1) steps
    print("# streams  us_per_step_off  us_per_step_on  extra_us  ratio  corners_kept_on   (1280x720, 48 corners, depth 0, %d steps per block, "
          "median of %d blocks, fb %.2f px)" % (args.steps, args.blocks, args.fb_px))
    for B in [int(x) for x in args.streams.split(",")]:
        frames = [torch.from_numpy(np.stack([seq.frame(k)] * B)).cuda().contiguous() for k in range(F)]
        c0 = torch.from_numpy(np.stack([seq.corners(0)] * B).astype(np.float32)).cuda().contiguous()
        trk = StreamTracker(1280, 720, seq.obj, seq.K, None, n_streams=B)
        trk.pipeline(0)
        so = trk.new_state_buffer()
        times = {0.0: [], args.fb_px: []}
        kept = 0
        for blk in range(2 * args.blocks):
            fb = args.fb_px if blk & 1 else 0.0
            trk.fb_check(fb)
            trk.reset(frames[0], c0)
            for i in range(args.warmup):
                trk.step(frames[walk[i % len(walk)]], so)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(args.warmup, args.warmup + args.steps):
                trk.step(frames[walk[i % len(walk)]], so)
            e1.record()
            torch.cuda.synchronize()
            times[fb].append(e0.elapsed_time(e1) * 1e3 / args.steps)
            if fb:
                kept = int(so.cpu().numpy()[:, H.ST_NTRACK].min())
        off, on = float(np.median(times[0.0])), float(np.median(times[args.fb_px]))
        print("%4d %12.2f %12.2f %9.2f %6.3f %6d" % (B, off, on, on - off, on / off, kept), flush=True)
        del trk, frames


if __name__ == "__main__":
    main()
