#!/usr/bin/env python
"""What the visibility rule of the reproject refresh is worth on a closed body, on the CPU (no GPU involved): the clips of
tests/visibility_scenes.py through the CPU oracle's LK + solvePnP(guess = previous pose) + the corner refresh, with the plain refresh
and with the refresh restricted to the tags the rule sees.  Frame 0 is what a detector delivers (the tags seen under the true pose).
Per run: the frames that pass the 2 px gate, the range of their mean reprojection error, the rotation gap to the truth at the last
frame, the tags that enter / leave the tracked set, and the least |cos - threshold| of any refresh.

    python tools/visibility_drift.py > profiles/tag_visibility_cpu.txt
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def chain(oracle, S, clip, view_deg, seed_deg):
    obj32 = clip.obj.astype(np.float32)
    obj = obj32.astype(np.float64)
    n = obj.shape[0]
    pts = clip.corners(0).copy()
    alive = clip.seed_mask(seed_deg).astype(bool)
    pose = clip.truth(0).copy()
    pyr = oracle.Pyramid(clip.frame(0), S.WIN, S.MAX_LEVEL)
    accepted, errs, margin, enter, leave = 0, [], np.inf, 0, 0
    tracked = alive.reshape(-1, 4).all(axis=1)
    for k in range(len(clip)):
        if k:
            npyr = oracle.Pyramid(clip.frame(k), S.WIN, S.MAX_LEVEL)
            nx, status, _ = oracle.calcOpticalFlowPyrLK(pyr, npyr, pts, winSize=(S.WIN, S.WIN), maxLevel=S.MAX_LEVEL)
            nx = nx.reshape(-1, 2).copy(); nx[~alive] = pts[~alive]
            alive = alive & status.ravel().astype(bool)
            pts = nx.astype(np.float32); pyr = npyr
        if alive.sum() < 8:
            continue
        r, t = pose[:3].copy(), pose[3:].copy()
        oracle.solvePnP(obj[alive], pts[alive].astype(np.float64), clip.K, None, r, t, True)
        cand = np.concatenate([r.ravel(), t.ravel()])
        err = oracle.mean_reproj_error(obj[alive], pts[alive].astype(np.float64), cand[:3], cand[3:], clip.K, None)
        if not err < 2.0:
            continue
        accepted += 1; errs.append(err); pose = cand
        pp, _ = oracle.projectPoints(obj, pose[:3], pose[3:], clip.K, None)
        pts = pp.reshape(-1, 2).astype(np.float32)
        if view_deg > 0:
            vis, cs, _ = S.tag_visibility(obj32, pose[:3], pose[3:], 4, view_deg, 1)
            margin = min(margin, float(np.abs(cs - S.cos_threshold(view_deg)).min()))
            alive = np.repeat(vis, 4)
            enter += int((vis & ~tracked).sum()); leave += int((~vis & tracked).sum())
            tracked = vis
        else:
            alive = np.ones(n, bool)
    gap = S.rotation_gap(pose[:3], clip.rvecs[len(clip) - 1])
    return dict(accepted=accepted, err=(min(errs), max(errs)) if errs else (np.nan, np.nan), gap=gap, enter=enter, leave=leave, margin=margin)


def main():
    from oracle import cvoracle as oracle
    import visibility_scenes as S
    oracle.build()
    print("# closed body, %d frames of %dx%d, %g deg per frame; chain: oracle LK + solvePnP(guess = previous pose) + refresh" %
          (S.N_FRAMES, S.WIDTH, S.HEIGHT, S.STEP_DEG))
    print("# tags step_deg view_deg  accepted  err_px_min err_px_max  rot_gap_rad  enter leave  margin")
    for T in (12, 24):
        for step in (S.STEP_DEG, -S.STEP_DEG):
            clip = S.ClosedBodyClip.get(T, step)
            for deg in (0.0, S.VIEW_DEG[T]):
                r = chain(oracle, S, clip, deg, S.VIEW_DEG[T])
                print("%5d %8g %8s  %3d / %2d  %10.3f %10.3f  %11.4f  %5d %5d  %s" %
                      (T, step, "off" if deg == 0 else "%g" % deg, r["accepted"], len(clip), r["err"][0], r["err"][1], r["gap"],
                       r["enter"], r["leave"], "-" if deg == 0 else "%.2e" % r["margin"]))


if __name__ == "__main__":
    main()
