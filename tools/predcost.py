#!/usr/bin/env python3
"""Cost of the motion-predicted initial flow (agt_tracker_predict, agt_predict_flow), measured with HIP events on one stream:

  frame   a stage-by-stage tracker frame (pipeline depth 0: pyramid -> [seed launch ->] LK -> pose step) at 48 corners with 1 and 64
          streams and at 240 corners with one stream, the option off and on, alternating block by block
  lk      the stand-alone LK launch on a frame pair of the fast 1280x720 scene (tests/predict_scenes.py FAST_720), started from the
          previous corners and from the seeds agt_predict_flow gives for the true poses of the two frames before
  call    agt_predict_flow itself at B = 1 and B = 64 (48 corners)

--package-root DIR times another checkout (the parent commit, say): a build without the option reports the off columns only.

    python tools/predcost.py [--steps 200] [--blocks 7] [--package-root DIR] [--label NAME]
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
    from accurate_aprilgroup_tracking_amd import hiplib as H, synthetic as syn
    from accurate_aprilgroup_tracking_amd import cv_hip
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    assert torch.cuda.is_available(), "needs a GPU"
    assert os.path.abspath(H.LIB_PATH).startswith(os.path.abspath(args.package_root)), H.LIB_PATH
    has = hasattr(StreamTracker, "predict")
    print("# %s (%s)" % (args.label, "with the option" if has else "no predict option in this build"))

    # ---- frame: a slow stream, so that every frame is accepted and (option on) every frame has a prediction
    for n_tags, B in ((12, 1), (12, 64), (60, 1)):
        seq = syn.Sequence(640, 480, n_tags=n_tags, n_frames=3, seed=0, supersample=2)
        frames = [torch.from_numpy(np.repeat(seq.frame(k)[None], B, axis=0)).cuda().contiguous() for k in range(3)]
        c0 = torch.from_numpy(np.repeat(seq.corners(0)[None].astype(np.float32), B, axis=0)).cuda().contiguous()
        trk = StreamTracker(640, 480, seq.obj, seq.K, None, n_streams=B)
        trk.pipeline(0)
        walk = [1, 2, 1, 0]
        state = {"i": 0}
        so = torch.zeros((B, H.STATE_STRIDE), dtype=torch.float64, device="cuda")

        def step():
            trk.step(frames[walk[state["i"] & 3]], so)
            state["i"] += 1
        res = {False: [], True: []}
        flow = None
        for blk in range(args.blocks):
            for on in ((False, True) if has else (False,)):
                if has:
                    trk.predict(64.0 if on else 0.0)
                trk.reset(frames[0], c0)
                state["i"] = 0
                res[on].append(timed(torch, step, args.steps, args.warmup))
                if on:
                    flow = so.cpu().numpy()[:, 15]
        line = "frame  %3d corners x %2d streams  off %.2f us (%.2f - %.2f)" % (4 * n_tags, B, np.median(res[False]), min(res[False]), max(res[False]))
        if has:
            line += "   on %.2f us (%.2f - %.2f)   +%.2f us   (last frame's flow_max %.2f .. %.2f px)" % (
                np.median(res[True]), min(res[True]), max(res[True]), np.median(res[True]) - np.median(res[False]), flow.min(), flow.max())
        print(line)
    if not has:
        return

    # ---- lk: the stand-alone launch on the fast scene, with and without seeds
    import predict_scenes as S
    w, h, seed, n_frames, A = S.FAST_720
    sc = S.FastSequence(w, h, seed, n_frames, A)
    ctx = cv_hip.Context(w, h, max_level=2, win=21, max_points=64, max_streams=1)
    obj = torch.from_numpy(sc.obj.astype(np.float32)).cuda().contiguous()
    for k in (3, 8):
        ctx.pyramid_build_pair(torch.from_numpy(sc.frame(k - 1)[None]).cuda().contiguous(), torch.from_numpy(sc.frame(k)[None]).cuda().contiguous())
        prev = torch.from_numpy(sc.corners(k - 1)[None].astype(np.float32)).cuda().contiguous()
        older = torch.from_numpy(sc.truth(k - 2)[None]).cuda().contiguous(); newer = torch.from_numpy(sc.truth(k - 1)[None]).cuda().contiguous()
        seeds, _, fmax, _ = ctx.predict_flow(obj, older, newer, sc.K, None, prev, None, 64.0)
        nxt = torch.zeros_like(prev)
        out = {}
        for name, start, flags in (("plain", prev, 0), ("seeded", seeds, H.LK_USE_INITIAL_FLOW)):
            def lk():
                nxt.copy_(start)
                return ctx.lk_track(0, 1, prev, nxt, flags=flags)

            def copy_only():
                nxt.copy_(start)
            ts = [timed(torch, lk, args.steps, args.warmup) - timed(torch, copy_only, args.steps, args.warmup) for _ in range(args.blocks)]
            res_lk = lk()
            torch.cuda.synchronize()
            err = np.abs(nxt.cpu().numpy()[0] - sc.corners(k)).max(axis=1)
            st = res_lk[1].cpu().numpy().ravel().astype(bool)
            out[name] = (np.median(ts), min(ts), max(ts), int(st.sum()), float(np.median(err)), float(err.max()))
        print("lk     FAST_720 frame %d (predicted flow_max %.1f px)  " % (k, float(fmax.cpu().numpy()[0])) +
              "   ".join("%s %.2f us (%.2f - %.2f), status 1 on %d / 48, corner error median %.2f max %.2f px" % ((name,) + out[name]) for name in out))

    # ---- call
    ctx = cv_hip.Context(64, 64, max_level=0, win=21, max_points=256, max_streams=64)
    for B in (1, 64):
        prev = torch.from_numpy(np.repeat(sc.corners(3)[None].astype(np.float32), B, axis=0)).cuda().contiguous()
        older = torch.from_numpy(np.repeat(sc.truth(2)[None], B, axis=0)).cuda().contiguous()
        newer = torch.from_numpy(np.repeat(sc.truth(3)[None], B, axis=0)).cuda().contiguous()
        ts = [timed(torch, lambda: ctx.predict_flow(obj, older, newer, sc.K, None, prev, None, 64.0), args.steps, args.warmup) for _ in range(args.blocks)]
        print("call   B = %2d  agt_predict_flow %.2f us (%.2f - %.2f; includes the Python wrapper's four allocations)" % (B, np.median(ts), min(ts), max(ts)))


if __name__ == "__main__":
    main()
