"""Scenes of the visibility rule's tests (test_tag_visibility.py, test_gpu_tag_visibility.py) and of tools/visibility_drift.py: seeded,
procedural.

A CLOSED body: `synthetic.make_april_group(max_polar_deg=180)` spreads T tags of 20 mm over a whole sphere, so at most about half of
them face the camera.  The clip turns the body about the camera's y axis by STEP degrees per frame in front of a static background:
    R_k = Ry(k * step) . R(rvec = R0),    t_k = T0 + k * DT,    k = 0 .. N_FRAMES - 1
at 640 x 480.  T = 12 gives 48 corners (the one-wave pose solve), T = 24 gives 96 (the cooperating-wave solve).  Tags cross the limb
during the clip: some leave the visible set, some enter it.

`tag_visibility` is the numpy statement of the rule in include/agt_hip.h (agt_tracker_visibility), `oracle_chain` the CPU chain the
tracker is held to: oracle LK + the PoseDetector mirror on the oracle backend + the reproject refresh with the rule, in Python.
"""
import json
import os

import numpy as np

WIDTH, HEIGHT = 640, 480
TAG_SIZE = 0.020
N_FRAMES = 16
STEP_DEG = 2.0
R0 = (0.2, -0.1, 0.3)
T0 = (0.01, -0.02, 0.30)
DT = (0.0004, 0.0003, 0.0005)
WIN, MAX_LEVEL = 21, 2
# tags of the body -> the view limit its tracker tests run at (degrees)
VIEW_DEG = {12: 75.0, 24: 70.0}


def cos_threshold(max_view_deg):
    """cos(max_view_deg), exactly 0 at 90 (cos(pi / 2) is 6e-17 in double): the plain back-face rule"""
    return 0.0 if max_view_deg == 90.0 else float(np.cos(np.deg2rad(max_view_deg)))


def tag_visibility(obj, rvec, tvec, cpt=4, max_view_deg=90.0, facing=1):
    """the rule of include/agt_hip.h in numpy float64 -> (visible (T,) bool, cos (T,) f64, centre depth c_c.z (T,) f64)"""
    from oracle import cvoracle
    R, _ = cvoracle.Rodrigues(np.asarray(rvec, np.float64).reshape(3))
    t = np.asarray(tvec, np.float64).reshape(3)
    p = np.asarray(obj).astype(np.float64).reshape(-1, cpt, 3)
    s = p[:, 0].copy()
    for k in range(1, cpt):                 # summed in index order
        s = s + p[:, k]
    c_o = s * (1.0 / cpt)
    n_o = facing * np.cross(p[:, 3] - p[:, 0], p[:, 1] - p[:, 0])
    c_c = c_o @ R.T + t
    n_c = n_o @ R.T
    with np.errstate(invalid="ignore", divide="ignore"):
        cs = -(n_c * c_c).sum(axis=1) / (np.sqrt((n_c * n_c).sum(axis=1)) * np.sqrt((c_c * c_c).sum(axis=1)))
        vis = (c_c[:, 2] > 0.0) & (cs > cos_threshold(max_view_deg))
    return vis, cs, c_c[:, 2]


class _Body:
    """model, payloads, camera and background of the T-tag closed body (shared by its clips)"""
    _cache = {}

    def __init__(self, n_tags):
        from accurate_aprilgroup_tracking_amd import synthetic as syn
        self.n_tags = n_tags
        self.group = syn.make_april_group(n_tags=n_tags, tag_size=TAG_SIZE, max_polar_deg=180, seed=0, sep=1.8)
        self.bits = syn.tag_bits(n_tags, 0)
        self.obj = syn.group_object_points(self.group)                # (4T, 3) f64
        self.K = syn.camera_matrix(WIDTH, HEIGHT)
        self.bg = syn.background(WIDTH, HEIGHT, 0)

    @classmethod
    def get(cls, n_tags):
        if n_tags not in cls._cache:
            cls._cache[n_tags] = cls(n_tags)
        return cls._cache[n_tags]


def clip_poses(step_deg, n_frames=N_FRAMES):
    """rvecs (F, 3), tvecs (F, 3) of the clip"""
    from scipy.spatial.transform import Rotation
    base = Rotation.from_rotvec(np.asarray(R0, np.float64))
    rv = np.stack([(Rotation.from_euler("y", k * step_deg, degrees=True) * base).as_rotvec() for k in range(n_frames)])
    tv = np.stack([np.asarray(T0, np.float64) + k * np.asarray(DT, np.float64) for k in range(n_frames)])
    return rv, tv


class ClosedBodyClip:
    """the interface of synthetic.Sequence (width, height, obj, K, dist, group, rvecs, tvecs, frame, corners) over the closed body"""
    _cache = {}

    def __init__(self, n_tags, step_deg=STEP_DEG, n_frames=N_FRAMES):
        body = _Body.get(n_tags)
        self.body, self.n_tags, self.step_deg = body, n_tags, step_deg
        self.width, self.height = WIDTH, HEIGHT
        self.group, self.bits, self.obj, self.K, self.dist, self.bg = body.group, body.bits, body.obj, body.K, None, body.bg
        self.rvecs, self.tvecs = clip_poses(step_deg, n_frames)
        self._frames = {}

    @classmethod
    def get(cls, n_tags, step_deg=STEP_DEG):
        key = (n_tags, step_deg)
        if key not in cls._cache:
            cls._cache[key] = cls(n_tags, step_deg)
        return cls._cache[key]

    def __len__(self):
        return self.rvecs.shape[0]

    def corners(self, k):
        """exact projections of ALL model corners at frame k (also those of the tags that face away), (4T, 2) float32"""
        from accurate_aprilgroup_tracking_amd import synthetic as syn
        return syn.project(self.obj, self.rvecs[k], self.tvecs[k], self.K, None).astype(np.float32)

    def frame(self, k, cover_out=None):
        from accurate_aprilgroup_tracking_amd import synthetic as syn
        if cover_out is not None:
            return syn.render_frame(self.group, self.bits, self.rvecs[k], self.tvecs[k], self.K, None, WIDTH, HEIGHT, self.bg, 1, cover_out=cover_out)
        if k not in self._frames:
            self._frames[k] = syn.render_frame(self.group, self.bits, self.rvecs[k], self.tvecs[k], self.K, None, WIDTH, HEIGHT, self.bg, 4)
        return self._frames[k]

    def truth(self, k):
        return np.concatenate([self.rvecs[k], self.tvecs[k]]).astype(np.float64)

    def seed_mask(self, view_deg):
        """what a detector delivers in frame 0: the corners of the tags the rule sees under the true pose, (4T,) u8"""
        vis, _, _ = tag_visibility(self.obj.astype(np.float32), self.rvecs[0], self.tvecs[0], 4, view_deg, 1)
        return np.repeat(vis, 4).astype(np.uint8)


def rotation_gap(rvec_a, rvec_b):
    """angle (rad) of the rotation that takes pose a's orientation to pose b's"""
    from scipy.spatial.transform import Rotation
    return float((Rotation.from_rotvec(np.asarray(rvec_a, np.float64).reshape(3)) *
                  Rotation.from_rotvec(np.asarray(rvec_b, np.float64).reshape(3)).inv()).magnitude())


def detector_class(tmp_dir, clip, tag):
    """the PoseDetector mirror with the clip's april_group.json"""
    from accurate_aprilgroup_tracking_amd.pose_detector import PoseDetector
    d = os.path.join(str(tmp_dir), "g_%s" % tag)
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "april_group.json"), "w") as f:
        f.write(json.dumps(clip.group))

    class Det(PoseDetector):
        DIRPATH = d
    return Det


def oracle_chain(oracle, clip, tmp_dir, tag, view_deg=0.0, fb_px=0.0, facing=1, log=None):
    """The CPU chain of one stream under reproject: frame 0 is detector-fed (the corners of seed_mask), frames 1.. are oracle LK from
    the refreshed corner set + PoseDetector._estimate_pose on the oracle backend; after an accepted pose the refresh is
    projectPoints(all object points) and -- view_deg > 0 -- the numpy rule on that pose (view_deg = 0: every corner revived);
    fb_px > 0: the forward-backward rule of tests/fb_scenes.py on every LK step.
    -> list of per-frame dicts: ntrack, ok, pose (6,) | None, nvisible, status (4T,) bool after the frame, margin (least
    |cos - threshold| of the refresh, inf without one), pts (4T, 2) f32 after the frame."""
    import logging
    from oracle import cv2_shim
    import fb_scenes
    if log is None:
        log = logging.getLogger("visibility_scenes"); log.setLevel(logging.CRITICAL)
    det = detector_class(tmp_dir, clip, tag)(log, clip.K, None, True, cv=cv2_shim.make_cv2())
    obj32 = clip.obj.astype(np.float32)
    n = obj32.shape[0]
    seed_deg = view_deg if view_deg > 0 else VIEW_DEG[clip.n_tags]
    pts = clip.corners(0).copy()
    alive = clip.seed_mask(seed_deg).astype(bool)
    pyr = oracle.Pyramid(clip.frame(0), WIN, MAX_LEVEL)
    out = []
    for k in range(len(clip)):
        if k:
            npyr = oracle.Pyramid(clip.frame(k), WIN, MAX_LEVEL)
            if fb_px > 0:
                nx, status, _, _, _ = fb_scenes.oracle_fb(oracle, pyr, npyr, pts, fb_px, win=(WIN, WIN), max_level=MAX_LEVEL, alive=alive)
            else:
                nx, status, _ = oracle.calcOpticalFlowPyrLK(pyr, npyr, pts, winSize=(WIN, WIN), maxLevel=MAX_LEVEL)
                nx = nx.reshape(-1, 2).copy(); nx[~alive] = pts[~alive]
            alive = alive & status.ravel().astype(bool)
            pts = nx.astype(np.float32); pyr = npyr
        il = [pts[j].reshape(1, 1, 2) for j in range(n) if alive[j]]
        ol = [obj32[j].reshape(1, 3) for j in range(n) if alive[j]]
        ntrack = len(il)
        det._estimate_pose(il if ntrack >= 8 else [], ol if ntrack >= 8 else [])
        solved = ntrack >= 8 and det.last_error is not None
        ok = bool(solved and det.last_error < 2)
        rec = dict(ntrack=ntrack, ok=ok, nvisible=0, margin=np.inf, err=det.last_error if solved else None,
                   pose=None if not solved else np.concatenate([det.last_pose[0].ravel(), det.last_pose[1].ravel()]).astype(np.float64))
        if ok:
            pp, _ = oracle.projectPoints(obj32.astype(np.float64), det.last_pose[0], det.last_pose[1], clip.K, None)
            pts = pp.reshape(-1, 2).astype(np.float32)
            if view_deg > 0:
                vis, cs, _ = tag_visibility(obj32, rec["pose"][:3], rec["pose"][3:], 4, view_deg, facing)
                alive = np.repeat(vis, 4)
                rec["nvisible"] = int(vis.sum())
                rec["margin"] = float(np.abs(cs - cos_threshold(view_deg)).min())
            else:
                alive = np.ones(n, bool)
        rec["status"] = alive.copy(); rec["pts"] = pts.copy()
        out.append(rec)
    return out
