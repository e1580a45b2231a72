#!/usr/bin/env python3
"""Calibrate the camera from a detection recording of a flat tag board: CameraParams.npz out of (recording, board, image size).

    python tools/calibrate_camera.py BOARD_REC.npz BOARD.json --size 1280 720 -o CameraParams.npz
    python tools/calibrate_camera.py BOARD_REC.npz BOARD.json --size 1280 720 --rational --fix-principal-point -o CameraParams.npz

BOARD_REC.npz: formats.save_detections of the board moved in front of the camera (tilt it: views parallel to the sensor carry no
focal length); BOARD.json: an april_group.json whose tags lie in one plane (sizes and positions as printed).  Writes mtx, dist and the
per-view rvecs, tvecs (formats.save_camera_params) and prints the report (INTEGRATION.md section 1i says how to read it).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("recording"); ap.add_argument("board")
    ap.add_argument("--size", type=int, nargs=2, required=True, metavar=("W", "H"), help="image size in pixels")
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
    frames = formats.load_detections(a.recording)
    with open(a.board) as f:
        board = json.load(f)
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
    obj, img, used = cc.target_points_from_detections(frames, board)
    rms, mtx, dist, rvecs, tvecs, report = cc.calibrate_camera(obj, img, tuple(a.size), mtx0, dist0, flags=flags, max_iters=a.max_iters)
    formats.save_camera_params(a.output, mtx, dist, rvecs.reshape(-1, 3, 1), tvecs.reshape(-1, 3, 1))
    print("frames of the recording with the board: %d of %d" % (len(used), len(frames)))
    print(cc.format_report(report))
    print("camera matrix      : fx %.4f fy %.4f cx %.4f cy %.4f" % (mtx[0, 0], mtx[1, 1], mtx[0, 2], mtx[1, 2]))
    print("distortion         : %s" % " ".join("%.6g" % v for v in dist.ravel()))
    print("wrote %s" % a.output)
    return 0


if __name__ == "__main__":
    sys.exit(main())
