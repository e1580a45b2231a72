#!/usr/bin/env python
"""Time of one agt_dense_model_accumulate call (profiles/dense_model.md): F resident 1280 x 720 frames, the 60-tag model at 32 x 32
(61,440 samples) and the 12-tag model beside it.  A host clock around the synchronous call, after a warm-up call.

The clip is eight rendered frames repeated F / 8 times with their poses: the kernel's work does not depend on what the pixels show.

    python tools/dense_model_time.py [--frames 256] [--repeat 5] [--statement] [--once]

--statement also times the numpy statement (tests/dense_model_numpy.py) on the same input and compares the sums;
--once makes one warm-up and one timed call per model (for a rocprofv3 --kernel-trace --stats run).
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--grid", type=int, default=32)
    ap.add_argument("--statement", action="store_true")
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    import torch
    from accurate_aprilgroup_tracking_amd import dense_model, synthetic
    W, H, F = 1280, 720, a.frames
    for n_tags in (60, 12):
        s = synthetic.Sequence(W, H, n_tags=n_tags, n_frames=8, seed=8, supersample=2)
        idx = np.arange(F) % 8
        frames_np = s.frames()[idx]
        poses = np.concatenate([s.rvecs, s.tvecs], axis=1)[idx]
        frames = torch.from_numpy(frames_np).cuda()
        xyz, tag, corners = dense_model.lattice(s.group, a.grid)
        M = xyz.shape[0]
        b = dense_model.DenseModelBuilder(s.K, None, W, H, corners, xyz, tag, 60.0, 1)
        b.begin_pass()
        obs = b.accumulate(frames, poses)                    # warm-up
        times = []
        for _ in range(1 if a.once else a.repeat):
            b.begin_pass()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            obs = b.accumulate(frames, poses)
            times.append(time.perf_counter() - t0)
        n, S, S2, rej = b.read()
        nobs = int(obs.sum())
        # shapes: every sample projects in every used frame; an observation reads four bytes of the frame
        flop_proj = 9 + 3 + 9 + 2 + 4 + 5      # R X (9 fma) + t, 1/z (Newton: ~9), x y, u v, z of the sample -- no distortion
        print("%d tags, M = %d, F = %d: accumulate %s ms (min %.3f); %d observations of %d sample-frames (%.1f %%)" %
              (n_tags, M, F, " ".join("%.3f" % (t * 1e3) for t in times), min(times) * 1e3, nobs, M * F, 100.0 * nobs / (M * F)))
        print("   by shape: %.1f M projections x ~%d FP64 operations = %.2f GFLOP; taps %.1f MB requested (4 B per sample-frame), sums %.1f MB "
              "(24 B read + 24 B written per sample), frames resident %.0f MB" %
              (M * F / 1e6, flop_proj, M * F * flop_proj / 1e9, M * F * 4 / 1e6, M * 48 / 1e6, frames_np.nbytes / 1e6))
        if a.statement:
            import dense_model_numpy as dm
            prob = dm.Problem(s.K, None, W, H, corners, xyz, tag, 60.0, 1)
            t0 = time.perf_counter()
            ref = dm.run_pass(prob, frames_np, poses)
            dt = time.perf_counter() - t0
            nn = np.maximum(ref["n"], 1)
            print("   numpy statement on the same input: %.2f s (one core); n equal: %s, max |S/n - statement| %.3g, max |S2/n - statement| %.3g" %
                  (dt, np.array_equal(n, ref["n"]), np.abs(S / nn - ref["S"] / nn).max(), np.abs(S2 / nn - ref["S2"] / nn).max()))
        b.close()


if __name__ == "__main__":
    main()
