"""Writes tests/golden/pose_range.npz: the inputs and the exact results (tests/pose_exact.py, mpmath, rounded once to float64) that
tests/test_gpu_pose_range.py holds the device code to.  Numbers only.  tests/test_pose_exact.py regenerates the table and compares
it bit for bit with the committed file.

    python tests/golden/make_pose_range_fixture.py

    K (3, 3), dist_mild (5,), dist_tilt14 (14,)                  the cameras
    theta (B,), pose (B, 6), obj (B, 6, 3)                       the ladder of rotations: B = 3 axes x 21 angles
    px_<cam>, jac_<cam>  (B, 6, 2), (B, 6, 2, 6)                 exact pixels and d(u, v)/d(rvec, tvec); cam: pinhole, mild, tilt14
    px32_<cam> (B, 6, 2)                                         exact pixels of the float32-rounded object points
    inv_older, inv_newer (M, 6), inv_kind (M,)                   agt_rodrigues_inv through agt_predict_flow; kind 0 zero rule, 1 pi, 2 generic
    inv_Rp (M, 3, 3), inv_tp (M, 3), inv_log (M, 3)              exact prediction and its exact rotation vector
    pnp_obj (12, 3), pnp_truth, pnp_guess (9, 6), pnp_img_<cam> (9, 12, 2)       noise-free projections for solvePnP; cam: pinhole, mild
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

PATH = os.path.join(HERE, "pose_range.npz")
KINDS = {"zero": 0, "pi": 1, "generic": 2}


def tables():
    import pose_exact as E
    out = {}
    _, theta, rvecs = E.ladder()
    obj = E.ladder_points(rvecs)
    B = len(theta)
    out["K"] = E.K; out["dist_mild"] = E.MILD_DIST; out["dist_tilt14"] = E.TILT14
    out["theta"] = theta
    out["pose"] = np.concatenate([rvecs, np.tile(E.TVEC, (B, 1))], axis=1)
    out["obj"] = obj
    names = list(E.CAMERAS)
    cams = [E.Camera(E.K, E.CAMERAS[c]) for c in names]
    for c in names:
        out["px_" + c] = np.empty((B, 6, 2)); out["jac_" + c] = np.empty((B, 6, 2, 6)); out["px32_" + c] = np.empty((B, 6, 2))
    obj32 = obj.astype(np.float32).astype(np.float64)
    for b in range(B):
        for c, (px, J) in zip(names, E.project(obj[b], rvecs[b], E.TVEC, cams, jacobian=True)):
            out["px_" + c][b] = E.f64(px); out["jac_" + c][b] = E.f64(J)
        for c, px in zip(names, E.project(obj32[b], rvecs[b], E.TVEC, cams)):
            out["px32_" + c][b] = E.f64(px)
    _, kinds, _, older, newer = E.inverse_ladder()
    M = len(kinds)
    out["inv_older"] = older; out["inv_newer"] = newer
    out["inv_kind"] = np.array([KINDS[k] for k in kinds], np.int32)
    out["inv_Rp"] = np.empty((M, 3, 3)); out["inv_tp"] = np.empty((M, 3)); out["inv_log"] = np.empty((M, 3))
    for m in range(M):
        Rp, tp = E.predict(older[m], newer[m])
        out["inv_Rp"][m] = E.f64(np.array(Rp.tolist(), object)); out["inv_tp"][m] = E.f64(tp); out["inv_log"][m] = E.f64(E.log_rotation(Rp))
    pobj, truth, guess = E.pnp_scene()
    out["pnp_obj"] = pobj; out["pnp_truth"] = truth; out["pnp_guess"] = guess
    pcams = [E.Camera(E.K, E.CAMERAS[c]) for c in ("pinhole", "mild")]
    for c in ("pinhole", "mild"):
        out["pnp_img_" + c] = np.empty((len(truth), len(pobj), 2))
    for q, p in enumerate(truth):
        for c, px in zip(("pinhole", "mild"), E.project(pobj, p[:3], p[3:], pcams)):
            out["pnp_img_" + c][q] = E.f64(px)
    return out


if __name__ == "__main__":
    t = tables()
    np.savez(PATH, **t)
    print("%s: %d arrays, %d bytes" % (PATH, len(t), os.path.getsize(PATH)))
