#!/usr/bin/env python3
"""Calibrate an AprilGroup from a detection recording: april_group.json out of (recording, camera, tag sizes).

    python tools/calibrate_group.py RECORDING.npz CameraParams.npz --sizes 0.02 -o april_group.json
    python tools/calibrate_group.py RECORDING.npz CameraParams.npz --sizes 0:0.02,1:0.02,7:0.015 --init nominal.json -o april_group.json

RECORDING.npz: formats.save_detections; CameraParams.npz: the reference's calibration file (mtx, dist).  --sizes: one edge length in
metres for every tag of the recording, or id:size pairs; with --init the sizes default to the nominal group's.  The anchor tag (default:
the one seen in the most frames) keeps its extrinsics -- the identity without --init, so the body frame is then that tag's frame.
Prints the report (INTEGRATION.md section 1g says how to read it).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_sizes(text, frames, init):
    from accurate_aprilgroup_tracking_amd import formats
    if text is None:
        if init is None:
            raise SystemExit("--sizes is needed without --init")
        return {int(k): float(v["size"]) for k, v in init["tags"].items()}
    if ":" in text:
        return {int(k): float(v) for k, v in (item.split(":") for item in text.split(","))}
    ids = sorted({int(d.tag_id) for dets in frames for d in dets if d.decision_margin >= formats.DECISION_MARGIN})
    return {t: float(text) for t in ids}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("recording"); ap.add_argument("camera")
    ap.add_argument("--sizes", help="edge length (m) of every tag, or id:size,id:size,...")
    ap.add_argument("--init", help="nominal april_group.json to start from")
    ap.add_argument("--anchor", type=int, help="tag id held fixed (default: the tag seen in the most frames)")
    ap.add_argument("--max-iters", type=int, default=50)
    ap.add_argument("--poses", help="write the per-frame body poses (rvecs, tvecs) to this .npz")
    ap.add_argument("-o", "--output", required=True)
    a = ap.parse_args(argv)
    import numpy as np
    from accurate_aprilgroup_tracking_amd import formats, group_calib
    frames = formats.load_detections(a.recording)
    mtx, dist, _, _ = formats.load_camera_params(a.camera)
    init = None
    if a.init:
        with open(a.init) as f:
            init = json.load(f)
    sizes = parse_sizes(a.sizes, frames, init)
    group, rvecs, tvecs, report = group_calib.calibrate_group(frames, sizes, mtx, dist, init_group=init, anchor=a.anchor, max_iters=a.max_iters)
    formats.save_april_group(a.output, group)
    if a.poses:
        np.savez(a.poses, rvecs=rvecs, tvecs=tvecs)
    print(group_calib.format_report(report))
    print("wrote %s (%d tags)" % (a.output, len(group["tags"])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
