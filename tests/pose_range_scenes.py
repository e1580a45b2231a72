"""Measures of the pose-range tests, and the scenes of the state-machine tests through R = I and through theta = pi (TEST
INFRASTRUCTURE; needs no mpmath).

A 12-tag group turns about the fixed general axis by 2 degrees per frame while it drifts in every component of the translation (the
reference's velocity buffers refuse a motion with a zero component, detect_pose.py:236); the angle is (k - 6.5) * 2 degrees past
the variant's centre, so the centre -- the identity, or the half turn -- lies midway between frames 6 and 7 of 14.  Corners are
noise-free.  `mirror_run` drives the PoseDetector mirror on the oracle backend over the scene and records what
tests/golden/make_reference_fixtures.py records of the reference: pose, guess, velocity buffers and acceptance per frame."""
import json
import logging
import os
import tempfile

import numpy as np

from accurate_aprilgroup_tracking_amd import synthetic

AXIS = np.array([0.6, -0.48, 0.64])
N_FRAMES, N_TAGS, STEP_DEG = 14, 12, 2.0
CENTRES = {"identity": 0.0, "pi": np.pi}
LOG = logging.getLogger("pose_range"); LOG.setLevel(logging.CRITICAL)


def rotation(rvec):
    t = float(np.linalg.norm(rvec))
    if t == 0.0:
        return np.eye(3)
    k = np.asarray(rvec, np.float64) / t
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(t) * Kx + (1.0 - np.cos(t)) * (Kx @ Kx)


FOCAL = 900.0          # of the ladder's camera (tests/pose_exact.py)


def block_ratios(J, Jx):
    """J, Jx (..., 2, 6): per point, the largest |J - Jx| of the rotation block and of the translation block, each over the largest
    |exact entry| of that block -> (..., 2).  A block that is exactly zero (the rotation block of the point at the origin) must be
    met exactly: its ratio is 0 or inf."""
    out = []
    for sl in (slice(0, 3), slice(3, 6)):
        d = np.abs(J[..., sl] - Jx[..., sl]).max(axis=(-1, -2))
        scale = np.abs(Jx[..., sl]).max(axis=(-1, -2))
        out.append(np.where(scale > 0, d / np.where(scale > 0, scale, 1.0), np.where(d == 0, 0.0, np.inf)))
    return np.stack(out, axis=-1)


def pixel_ratios(px, pxx):
    return np.abs(px - pxx).max(axis=-1) / np.maximum(np.abs(pxx).max(axis=-1), FOCAL)


class TurnScene:
    def __init__(self, variant):
        self.group = synthetic.make_april_group(n_tags=N_TAGS, seed=17)
        self.K = synthetic.camera_matrix(1280, 720)
        self.dist = None
        k = np.arange(N_FRAMES)
        self.theta = CENTRES[variant] + (k - 6.5) * np.deg2rad(STEP_DEG)
        self.rvecs = self.theta[:, None] * AXIS
        self.tvecs = np.array([0.01, -0.02, 0.35]) + k[:, None] * np.array([0.0007, -0.0005, 0.0011])
        obj = synthetic.group_object_points(self.group)
        self.corners = np.empty((N_FRAMES, 4 * N_TAGS, 2))
        for f in range(N_FRAMES):
            Y = obj @ rotation(self.rvecs[f]).T + self.tvecs[f]
            assert (Y[:, 2] > 0.2).all()
            self.corners[f] = Y[:, :2] / Y[:, 2:] * self.K[0, 0] + self.K[:2, 2]


def mirror_run(scene):
    """-> dict of per-frame arrays: pose (F, 6), pose_valid, guess (F, 6), guess_valid, n_vel, rot_vel (F, 2, 9), tran_vel (F, 2, 3),
    prev (F, 6), prev_valid; and all_objpts (the mirror's float32-built object points)"""
    from oracle import cv2_shim
    from accurate_aprilgroup_tracking_amd.pose_detector import PoseDetector
    tmp = tempfile.mkdtemp()
    with open(os.path.join(tmp, "april_group.json"), "w") as f:
        json.dump(scene.group, f)

    class Det(PoseDetector):
        DIRPATH = tmp
    det = Det(LOG, scene.K, scene.dist, True, cv=cv2_shim.make_cv2())
    tag_ids = sorted(det.extrinsics)
    rec = {k: [] for k in ("pose", "pose_valid", "guess", "guess_valid", "prev", "prev_valid", "n_vel", "rot_vel", "tran_vel")}

    def pack(tr):
        if tr[0] is None:
            return np.zeros(6), 0
        return np.concatenate([np.asarray(tr[0], np.float64).ravel(), np.asarray(tr[1], np.float64).ravel()]), 1
    for k in range(N_FRAMES):
        img_list, obj_list = [], []
        for t, tid in enumerate(tag_ids):
            size, tvec, rvec = det.extrinsics[tid][:3]
            img_list.append(scene.corners[k, 4 * t:4 * t + 4].reshape(1, 4, 2))
            obj_list.append(det.transform_marker_corners(det.get_initial_pts(size), (rvec, tvec)))
        before = det.prev_transform
        det._estimate_pose(img_list, obj_list)
        accepted = det.prev_transform is not before
        v, ok = pack(det.prev_transform if accepted else (None, None)); rec["pose"].append(v); rec["pose_valid"].append(ok)
        v, ok = pack(det.extrinsic_guess); rec["guess"].append(v); rec["guess_valid"].append(ok)
        v, ok = pack(det.prev_transform); rec["prev"].append(v); rec["prev_valid"].append(ok)
        nv = len(det.rot_velocities); rec["n_vel"].append(nv)
        rvb = np.zeros((2, 9)); tvb = np.zeros((2, 3))
        for i in range(nv):
            rvb[i] = np.asarray(det.rot_velocities[i]).ravel(); tvb[i] = np.asarray(det.tran_velocities[i]).ravel()
        rec["rot_vel"].append(rvb); rec["tran_vel"].append(tvb)
    out = {k: np.array(v) for k, v in rec.items()}
    out["all_objpts"] = np.asarray(det.all_objpts)
    return out


def guess_sign_changes(rec):
    """how often the guess's rotation vector changes side of the plane normal to the axis, over the frames that have a guess"""
    s = [np.sign(g[:3] @ AXIS) for g, ok in zip(rec["guess"], rec["guess_valid"]) if ok]
    return int(sum(a != b for a, b in zip(s[:-1], s[1:])))
