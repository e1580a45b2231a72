#!/usr/bin/env python3
"""Calibrate the camera from a detection recording of a flat tag board: CameraParams.npz out of (recording, board, image size).

    python tools/calibrate_camera.py BOARD_REC.npz BOARD.json --size 1280 720 -o CameraParams.npz
    python tools/calibrate_camera.py BOARD_REC.npz BOARD.json --size 1280 720 --rational --fix-principal-point -o CameraParams.npz
    python tools/calibrate_camera.py --chessboard 9 6 --square 0.025 FRAMES.npz -o CameraParams.npz

BOARD_REC.npz: formats.save_detections of the board moved in front of the camera (tilt it: views parallel to the sensor carry no
focal length); BOARD.json: an april_group.json whose tags lie in one plane (sizes and positions as printed).  Writes mtx, dist and the
per-view rvecs, tvecs (formats.save_camera_params) and prints the report (INTEGRATION.md section 1i says how to read it).

--chessboard NX NY --square S: the second input form, photographs of a printed chessboard with NX x NY inner corners and squares of
side S.  FRAMES is a .npy or .npz stack of gray (V, H, W) or BGR (V, H, W, 3) u8 frames, or image files,
which are read through PIL when it is installed; no board file and no --size are needed.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def load_frames(paths, fail):
    """.npy / .npz stacks and image files -> list of (H, W) or (H, W, 3) u8 frames of one size"""
    import numpy as np
    frames = []
    for p in paths:
        ext = os.path.splitext(p)[1].lower()
        if ext == ".npy":
            stacks = [np.load(p)]
        elif ext == ".npz":
            with np.load(p) as z:
                stacks = [z[k] for k in z.files]
        else:
            try:
                from PIL import Image
            except ImportError:
                fail("%s is an image file and reading it needs the module PIL, which is not installed; "
                     "convert the frames to a .npy or .npz stack" % p)
            stacks = [np.asarray(Image.open(p).convert("L"))[None]]
        for s in stacks:
            s = np.asarray(s)
            if s.dtype != np.uint8 or s.ndim not in (2, 3, 4) or (s.ndim == 4 and s.shape[3] != 3):
                fail("%s: frames must be u8 (H, W), (V, H, W) or (V, H, W, 3), not %s %s" % (p, s.dtype, s.shape))
            frames += list(s[None] if s.ndim == 2 else s)
    if not frames or any(f.shape[:2] != frames[0].shape[:2] for f in frames):
        fail("the frames must all have one size")
    return frames


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("recording", nargs="+", help="the detection recording and the board's json, or with --chessboard the frames")
    ap.add_argument("--size", type=int, nargs=2, metavar=("W", "H"), help="image size in pixels (taken from the frames with --chessboard)")
    ap.add_argument("--chessboard", type=int, nargs=2, metavar=("NX", "NY"), help="inner corners per row and column of a chessboard")
    ap.add_argument("--square", type=float, help="side of a chessboard square, in the unit the poses shall have")
    ap.add_argument("-o", "--output", default="CameraParams.npz")
    ap.add_argument("--guess", help="CameraParams.npz to start from (CALIB_USE_INTRINSIC_GUESS)")
    ap.add_argument("--rational", action="store_true", help="estimate k4 k5 k6 (8 coefficients)")
    ap.add_argument("--thin-prism", action="store_true", help="estimate s1 s2 s3 s4 (12 coefficients)")
    ap.add_argument("--zero-tangent", action="store_true", help="p1 = p2 = 0")
    ap.add_argument("--fix-principal-point", action="store_true")
    ap.add_argument("--fix-focal-length", action="store_true", help="with --guess")
    ap.add_argument("--fix-k", type=int, nargs="*", default=[], choices=range(1, 7), metavar="N", help="hold k_N (1..6)")
    ap.add_argument("--max-iters", type=int, default=100)
    a = ap.parse_args(argv)
    from accurate_aprilgroup_tracking_amd import camera_calib as cc, formats
    if a.chessboard:
        if a.square is None or not a.square > 0:
            ap.error("--chessboard needs --square S > 0")
        frames = load_frames(a.recording, ap.error)
        size = (frames[0].shape[1], frames[0].shape[0])
    else:
        if len(a.recording) != 2 or a.size is None:
            ap.error("a detection recording needs RECORDING BOARD --size W H")
        frames = formats.load_detections(a.recording[0])
        with open(a.recording[1]) as f:
            board = json.load(f)
        size = tuple(a.size)
    flags = 0
    mtx0 = dist0 = None
    if a.guess:
        mtx0, dist0, _, _ = formats.load_camera_params(a.guess)
        flags |= cc.CALIB_USE_INTRINSIC_GUESS
    for on, bit in ((a.rational, cc.CALIB_RATIONAL_MODEL), (a.thin_prism, cc.CALIB_THIN_PRISM_MODEL), (a.zero_tangent, cc.CALIB_ZERO_TANGENT_DIST),
                    (a.fix_principal_point, cc.CALIB_FIX_PRINCIPAL_POINT), (a.fix_focal_length, cc.CALIB_FIX_FOCAL_LENGTH)):
        if on:
            flags |= bit
    for k in a.fix_k:
        flags |= (cc.CALIB_FIX_K1, cc.CALIB_FIX_K2, cc.CALIB_FIX_K3, cc.CALIB_FIX_K4, cc.CALIB_FIX_K5, cc.CALIB_FIX_K6)[k - 1]
    if a.chessboard:
        obj, img, used = cc.target_points_from_chessboards(frames, tuple(a.chessboard), a.square)
    else:
        obj, img, used = cc.target_points_from_detections(frames, board)
    rms, mtx, dist, rvecs, tvecs, report = cc.calibrate_camera(obj, img, size, mtx0, dist0, flags=flags, max_iters=a.max_iters)
    formats.save_camera_params(a.output, mtx, dist, rvecs.reshape(-1, 3, 1), tvecs.reshape(-1, 3, 1))
    print("frames of the recording with the board: %d of %d" % (len(used), len(frames)))
    print(cc.format_report(report))
    print("camera matrix      : fx %.4f fy %.4f cx %.4f cy %.4f" % (mtx[0, 0], mtx[1, 1], mtx[0, 2], mtx[1, 2]))
    print("distortion         : %s" % " ".join("%.6g" % v for v in dist.ravel()))
    print("wrote %s" % a.output)
    return 0


if __name__ == "__main__":
    sys.exit(main())
