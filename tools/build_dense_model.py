#!/usr/bin/env python
"""Learn the dense model's template from a recording: frames + poses -> a .npz that StreamTracker.load_dense_model reads.

    python tools/build_dense_model.py --group april_group.json --camera CameraParams.npz --frames frames.npy --poses poses.npy \\
        [--use use.npy] --grid 32 --out dense_model.npz

Frames are a (F, H, W) uint8 .npy of gray frames, memory-mapped and uploaded in chunks (there is no video decoder here: decode the
recording to that array first).  Poses are (F, 6) float64, rvec | tvec of the body in each frame -- the accepted records of the
tracker (slots 0..5 of a state record whose gate passed) or the frame poses calibrate_group returns; --use marks the frames to take.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--group", required=True, help="april_group.json")
    ap.add_argument("--camera", required=True, help="CameraParams.npz (mtx, dist)")
    ap.add_argument("--frames", required=True, help="(F, H, W) uint8 .npy, memory-mapped; no video decoder exists here")
    ap.add_argument("--poses", required=True, help="(F, 6) float64 .npy: rvec | tvec per frame")
    ap.add_argument("--use", help="(F,) .npy: non-zero = take the frame (default: all)")
    ap.add_argument("--grid", type=int, default=32, help="lattice points per tag edge")
    ap.add_argument("--extent", type=float, default=0.6)
    ap.add_argument("--max-view-deg", type=float, default=60.0)
    ap.add_argument("--facing", type=int, default=1, choices=(1, -1))
    ap.add_argument("--clip-sigma", type=float, default=1.5, help="0: no clipped pass")
    ap.add_argument("--sigma-floor", type=float, default=4.0)
    ap.add_argument("--min-obs", type=int, default=4)
    ap.add_argument("--max-std", type=float, default=float("inf"))
    ap.add_argument("--out", required=True, help="the dense model (.npz)")
    a = ap.parse_args(argv)

    from accurate_aprilgroup_tracking_amd import dense_model, formats
    group = formats.load_april_group(a.group)
    K, dist, _, _ = formats.load_camera_params(a.camera)
    frames = np.load(a.frames, mmap_mode="r")
    poses = np.load(a.poses)
    use = np.load(a.use) if a.use else None
    if frames.ndim != 3 or frames.dtype != np.uint8:
        ap.error("--frames must hold a (F, H, W) uint8 array")
    if poses.shape != (frames.shape[0], 6):
        ap.error("--poses must hold a (%d, 6) array" % frames.shape[0])
    model = dense_model.build_dense_model(frames, poses, group, K, dist, use=use, grid=a.grid, extent=a.extent, max_view_deg=a.max_view_deg,
                                          facing=a.facing, clip_sigma=a.clip_sigma, sigma_floor=a.sigma_floor, min_obs=a.min_obs,
                                          max_std=a.max_std)
    formats.save_dense_model(a.out, model)
    print(model.report())
    print("wrote %s" % a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
