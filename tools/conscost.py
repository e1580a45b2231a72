#!/usr/bin/env python3
"""Cost of the tag-consensus option (agt_tracker_consensus, agt_solve_pnp_consensus), measured with HIP events on one stream:

  frame   a stage-by-stage tracker frame (pyramid -> LK -> backward LK -> [hypotheses -> vote ->] pose step; fb_check on, which is the
          stage-by-stage yardstick) at 48 and 240 corners, the option off and on, alternating block by block
  call    the stateless call at B = 1 and B = 64 (48 corners) against one plain agt_solve_pnp with a guess
  scene   pose error and acceptance on the sliding-tags scene of tests/consensus_scenes.py, with and without the option

--package-root DIR times another checkout (the parent commit, say): a build without the option reports the off columns only.

    python tools/conscost.py [--steps 200] [--blocks 7] [--package-root DIR] [--label NAME]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(torch, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--label", default="this tree")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch
    from oracle import cvoracle
    cvoracle.build()
    import consensus_scenes as S
    from accurate_aprilgroup_tracking_amd import hiplib as H, synthetic as syn
    from accurate_aprilgroup_tracking_amd import cv_hip
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    assert torch.cuda.is_available(), "needs a GPU"
    assert os.path.abspath(H.LIB_PATH).startswith(os.path.abspath(args.package_root)), H.LIB_PATH
    has = hasattr(StreamTracker, "consensus")
    print("# %s (%s)" % (args.label, "with the option" if has else "no consensus option in this build"))

    # ---- frame
    for n_tags in (12, 60):
        seq = syn.Sequence(640, 480, n_tags=n_tags, n_frames=3, seed=0, supersample=2)
        frames = [torch.from_numpy(seq.frame(k)[None]).cuda().contiguous() for k in range(3)]
        c0 = torch.from_numpy(seq.corners(0)[None].astype(np.float32)).cuda().contiguous()
        trk = StreamTracker(640, 480, seq.obj, seq.K, None, n_streams=1, fb_check=1.0)
        trk.pipeline(0)
        walk = [1, 2, 1, 0]
        state = {"i": 0}

        def step():
            trk.step(frames[walk[state["i"] & 3]])
            state["i"] += 1
        res = {False: [], True: []}
        for blk in range(args.blocks):
            for on in ((False, True) if has else (False,)):
                if has:
                    trk.consensus(2.0 if on else 0.0)
                trk.reset(frames[0], c0)
                state["i"] = 0
                res[on].append(timed(torch, step, args.steps, args.warmup))
        line = "frame  %3d corners  off %.2f us (%.2f - %.2f)" % (4 * n_tags, np.median(res[False]), min(res[False]), max(res[False]))
        if has:
            line += "   on %.2f us (%.2f - %.2f)   +%.2f us" % (np.median(res[True]), min(res[True]), max(res[True]), np.median(res[True]) - np.median(res[False]))
        print(line)

    # ---- call
    ctx = cv_hip.Context(64, 64, max_level=0, win=21, max_points=256, max_streams=64)
    sc = S.Scene(12, 1, 3, group_seed=0)
    for B in (1, 64):
        obj = torch.from_numpy(sc.obj).cuda().contiguous()
        img = torch.from_numpy(np.repeat(sc.img()[None], B, axis=0)).cuda().contiguous()
        guess = torch.from_numpy(np.repeat(sc.guess[None], B, axis=0)).cuda().contiguous()
        pose = guess.clone()

        def plain():
            pose.copy_(guess)
            ctx.solve_pnp(obj, img, sc.K, sc.dist, pose, True)

        def cons():
            pose.copy_(guess)
            ctx.solve_pnp_consensus(obj, img, sc.K, sc.dist, pose, True)

        def copy_only():
            pose.copy_(guess)
        res = {"copy": [], "plain": [], "cons": []}
        for blk in range(args.blocks):
            res["copy"].append(timed(torch, copy_only, args.steps, args.warmup))
            res["plain"].append(timed(torch, plain, args.steps, args.warmup))
            if has:
                res["cons"].append(timed(torch, cons, args.steps, args.warmup))
        cp = np.median(res["copy"])
        line = "call   B = %2d  plain agt_solve_pnp %.2f us" % (B, np.median(res["plain"]) - cp)
        if has:
            line += "   agt_solve_pnp_consensus %.2f us   (each without the %.2f us guess copy; includes the Python wrapper's four allocations)" % (np.median(res["cons"]) - cp, cp)
        print(line)

    # ---- scene
    scn = S.SlidingSequence()
    steps = len(scn) - 1
    truth = np.stack([scn.truth(k) for k in range(1, steps + 1)])
    for on in ((False, True) if has else (False,)):
        kw = dict(consensus_px=2.0) if on else {}
        trk = StreamTracker(scn.width, scn.height, scn.obj, scn.K, scn.dist, n_streams=1, **kw)
        trk.pipeline(0)
        trk.reset(torch.from_numpy(scn.frame(0)[None]).cuda().contiguous(), torch.from_numpy(scn.corners(0)[None].astype(np.float32)).cuda().contiguous())
        so = torch.zeros((steps, 1, H.STATE_STRIDE), dtype=torch.float64, device="cuda")
        for i in range(steps):
            trk.step(torch.from_numpy(scn.frame(i + 1)[None]).cuda().contiguous(), so[i])
        torch.cuda.synchronize()
        r = so.cpu().numpy()[:, 0]
        print("scene  option %-3s accepted %d / %d   reprojection error %s   |rvec - truth| %s" %
              ("on" if on else "off", int(r[:, H.ST_OK].sum()), steps, np.round(r[:, H.ST_ERR], 3).tolist(),
               np.round(np.abs(r[:, :3] - truth[:, :3]).max(axis=1), 5).tolist()))


if __name__ == "__main__":
    main()
