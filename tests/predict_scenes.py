"""Scenes of the motion-predicted initial flow's tests (test_predict_flow.py, test_gpu_predict_flow.py): seeded, procedural.

A `FastSequence` is a `synthetic.Sequence` of 12 tags (48 corners) whose trajectory is replaced, before any frame is rendered, by a
sweep that starts at rest and accelerates -- the image motion passes the ~15 px per frame that LK reaches from a standing start within
three frames and keeps growing (FAST_480: 40 px per frame, FAST_720: 53).  `flow_rule` is the numpy statement of the seed rule of
include/agt_hip.h (agt_predict_flow) on `oracle.Rodrigues` / `oracle.projectPoints`: the expected value of every test.
"""
import json

import numpy as np

WIN, MAX_LEVEL = 21, 2
CAP_PX = 64.0
# (width, height, seed, frames, amplitude A of the sweep in metres)
FAST_480 = (640, 480, 3, 10, (0.09, 0.03, 0.02))
FAST_720 = (1280, 720, 1, 10, (0.06, 0.02, 0.02))


def fast_trajectory(n_frames, A):
    k = np.arange(n_frames, dtype=np.float64)[:, None]
    A = np.asarray(A, np.float64)
    tv = (np.array([0.01, -0.02, 0.30]) + A * (1.0 - np.cos(2 * np.pi * k / np.array([32.0, 41.0, 53.0]))) * np.array([1.0, -1.0, 1.0])
          - np.array([A[0], -A[1], 0.0]))
    rv = np.array([0.2, -0.1, 0.3]) + np.array([0.08, 0.10, 0.06]) * np.sin(2 * np.pi * k / np.array([37.0, 45.0, 51.0])) ** 2
    return rv, tv


class FastSequence:
    """frames / corners / truth of a synthetic.Sequence on the fast trajectory"""

    def __init__(self, width, height, seed, n_frames, A):
        from accurate_aprilgroup_tracking_amd import synthetic as syn
        self.seq = syn.Sequence(width, height, n_tags=12, n_frames=n_frames, seed=seed)
        self.seq.rvecs, self.seq.tvecs = fast_trajectory(n_frames, A)        # (before any frame is rendered: frames are lazy)
        self.width, self.height = width, height
        self.obj, self.K, self.dist, self.group = self.seq.obj, self.seq.K, self.seq.dist, self.seq.group
        self.rvecs, self.tvecs = self.seq.rvecs, self.seq.tvecs

    def __len__(self):
        return len(self.seq)

    def corners(self, k):
        return self.seq.corners(k)

    def frame(self, k):
        return self.seq.frame(k)

    def truth(self, k):
        return np.concatenate([self.rvecs[k].ravel(), self.tvecs[k].ravel()]).astype(np.float64)


_scenes = {}


def scene(spec):
    """one FastSequence per specification and session: its frames are rendered once"""
    if spec not in _scenes:
        _scenes[spec] = FastSequence(*spec)
    return _scenes[spec]


def flow_rule(oracle, obj, prev, older, newer, K, dist, usable=None, cap=CAP_PX):
    """include/agt_hip.h agt_predict_flow for one stream: obj (n,3) as the device holds it (float32 or float64), prev (n,2) float32,
    older / newer (6,) float64 -> (seeds (n,2) f32, flow (n,2) f32, flow_max, pose_pred (6,) f64)"""
    prev = np.ascontiguousarray(np.asarray(prev, np.float32).reshape(-1, 2))
    n = prev.shape[0]
    obj64 = np.asarray(obj).reshape(n, 3).astype(np.float64)
    usable = np.ones(n, bool) if usable is None else np.asarray(usable).reshape(n) != 0
    older = np.asarray(older, np.float64).reshape(6); newer = np.asarray(newer, np.float64).reshape(6)
    distrusted = (prev.copy(), np.zeros((n, 2), np.float32), -1.0)
    if not (np.isfinite(older).all() and np.isfinite(newer).all()):
        return distrusted + (np.full(6, np.nan),)
    R2 = np.asarray(oracle.Rodrigues(older[:3].reshape(3, 1))[0], np.float64)
    R1 = np.asarray(oracle.Rodrigues(newer[:3].reshape(3, 1))[0], np.float64)
    t2, t1 = older[3:], newer[3:]
    D = R1 @ R2.T
    Rp = D @ R1
    tp = D @ (t1 - t2) + t1
    rp = np.asarray(oracle.Rodrigues(Rp)[0], np.float64).reshape(3)
    pred = np.concatenate([rp, tp])
    p1 = np.asarray(oracle.projectPoints(obj64, newer[:3].reshape(3, 1), t1.reshape(3, 1), K, dist)[0], np.float64).reshape(n, 2)
    pp = np.asarray(oracle.projectPoints(obj64, rp.reshape(3, 1), tp.reshape(3, 1), K, dist)[0], np.float64).reshape(n, 2)
    with np.errstate(over="ignore", invalid="ignore"):
        flow = (pp - p1).astype(np.float32)
    Rpp = np.asarray(oracle.Rodrigues(rp.reshape(3, 1))[0], np.float64)
    z1 = obj64 @ R1[2] + t1[2]; zp = obj64 @ Rpp[2] + tp[2]
    mag = np.abs(flow).max(axis=1)
    with np.errstate(invalid="ignore"):
        fine = (z1 > 0) & (zp > 0) & np.isfinite(flow).all(axis=1) & (mag <= np.float32(cap))
    if not fine[usable].all():
        return distrusted + (pred,)
    flow[~usable] = 0.0
    seeds = prev.copy()
    seeds[usable] = prev[usable] + flow[usable]
    return seeds, flow, float(mag[usable].max()) if usable.any() else 0.0, pred


class FirstFrameDetector:
    """every tag in the first frame, nothing afterwards: the LK path carries the stream"""

    def __init__(self, sc):
        from accurate_aprilgroup_tracking_amd import formats
        self.sc, self.k, self.F = sc, 0, formats
        self.tag_ids = [int(t) for t in sc.group["tags"].keys()]

    def __call__(self, gray):
        k = self.k
        self.k += 1
        if k:
            return []
        c = self.sc.corners(0).reshape(-1, 4, 2)
        return [self.F.make_detection(t, c[i], decision_margin=75.0) for i, t in enumerate(self.tag_ids)]


def detector_class(tmp_path, sc, tag):
    from accurate_aprilgroup_tracking_amd.pose_detector import PoseDetector
    d = tmp_path / ("g_%s" % tag)
    d.mkdir(exist_ok=True)
    (d / "april_group.json").write_text(json.dumps(sc.group))

    class Det(PoseDetector):
        DIRPATH = str(d)
    return Det
