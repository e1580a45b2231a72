#!/usr/bin/env python3
"""Tabulates tests/golden/rodrigues_tiny.npz from tests/pose_exact.py (mpmath): exact pixels and Jacobians of six points under four
rotation vectors at and below DBL_EPSILON -- where agt_rodrigues (csrc/agt_device.h) takes its R = I case -- for the three cameras of
the pose ladder.  tests/test_gpu_rodrigues_tiny.py reads only the table.

    python tests/golden/make_rodrigues_tiny_fixture.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import pose_exact as px        # noqa: E402

RVECS = np.array([[0.0, 0.0, 0.0],
                  [1e-17, 0.0, 0.0],
                  3e-16 * np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0),
                  [0.0, 0.0, 1e-12]])


def main():
    obj = px.ladder_points(RVECS)
    cams = [px.Camera(px.K, d) for d in px.CAMERAS.values()]
    out = {"rvec": RVECS, "pose": np.concatenate([RVECS, np.tile(px.TVEC, (len(RVECS), 1))], axis=1), "obj": obj, "K": px.K,
           "theta": np.linalg.norm(RVECS, axis=1)}
    for name, d in px.CAMERAS.items():
        if d is not None:
            out["dist_" + name] = d
        out["px_" + name] = np.empty((len(RVECS), 6, 2))
        out["jac_" + name] = np.empty((len(RVECS), 6, 2, 6))
    for b, r in enumerate(RVECS):
        res = px.project(obj[b], r, px.TVEC, cams, jacobian=True)
        for name, (p, J) in zip(px.CAMERAS, res):
            out["px_" + name][b] = px.f64(p)
            out["jac_" + name][b] = px.f64(J)
    np.savez(os.path.join(HERE, "rodrigues_tiny.npz"), **out)
    print("wrote rodrigues_tiny.npz: %d rotations, %d cameras" % (len(RVECS), len(cams)))


if __name__ == "__main__":
    main()
