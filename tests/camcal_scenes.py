"""Scene builders of the camera-calibration tests (TEST INFRASTRUCTURE): views of a planar target, tilted 17-35 degrees against the
sensor about a random in-plane axis and rolled up to 20 degrees, projected with tests/pnp_numpy.project under a known camera vector
c[16] = fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 (noise-free, or with seeded Gaussian noise)."""
import numpy as np
from scipy.spatial.transform import Rotation

from accurate_aprilgroup_tracking_amd import formats

import camera_calib_numpy as cn

SIZE = (640, 480)
# every entry non-zero
CAM12 = np.array([520.0, 515.0, 325.0, 238.0, -0.12, 0.05, 1e-3, -8e-4, -0.01, 0.02, -0.01, 0.005, 1e-3, -5e-4, 5e-4, 1e-3])
CAM8 = np.concatenate([CAM12[:12], np.zeros(4)])
CAM5 = np.concatenate([CAM12[:9], np.zeros(7)])
FREE5 = list(range(9))                               # fx fy cx cy k1 k2 p1 p2 k3
FREE8 = list(range(12))                              # ... k4 k5 k6: near-singular on a 9 x 6 board at 12 views (see test_gpu_camera_calib.py)
FREE_PRISM = list(range(9)) + [12, 13, 14, 15]       # 4 + 5 + 4: the thin-prism set with k4 k5 k6 held


def grid(nx, ny, pitch):
    """(nx ny, 3) grid points in the plane z = 0, centred"""
    x, y = np.meshgrid((np.arange(nx) - (nx - 1) / 2.0) * pitch, (np.arange(ny) - (ny - 1) / 2.0) * pitch)
    return np.stack([x.ravel(), y.ravel(), np.zeros(nx * ny)], axis=1)


def view_poses(n, extent, cam, size, rng, tilt_deg=(17.0, 35.0), fill=0.7):
    """n poses target -> camera: the target's largest extent fills `fill` of the image width (a tilted corner may leave the frame by a
    few pixels: the points are projected, not cropped), its centre up to 8 % of the extent off the axis.  At fill = 0.55 the thin-prism
    set's Schur and dense steps differ by 9e-9 in numpy itself; 0.7 leaves the 1e-8 of the CPU test a factor of ten"""
    poses = []
    for _ in range(n):
        th = np.deg2rad(rng.uniform(*tilt_deg)); ph = rng.uniform(0, 2 * np.pi); roll = np.deg2rad(rng.uniform(-20, 20))
        R = Rotation.from_rotvec([0, 0, roll]).as_matrix() @ Rotation.from_rotvec(th * np.array([np.cos(ph), np.sin(ph), 0.0])).as_matrix()
        d = cam[0] * extent / (fill * size[0])
        t = np.array([rng.uniform(-0.08, 0.08) * extent, rng.uniform(-0.08, 0.08) * extent, d * rng.uniform(0.9, 1.15)])
        poses.append(np.concatenate([Rotation.from_matrix(R).as_rotvec(), t]))
    return np.array(poses)


class Scene:
    """obj / img: per-view point lists; cam: the true camera vector; poses: the true view poses (V, 6)"""

    def __init__(self, targets, cam, seed, noise=0.0, size=SIZE, tilt_deg=(17.0, 35.0), poses=None, fill=0.7):
        rng = np.random.default_rng(seed)
        self.size, self.cam = size, np.array(cam, np.float64)
        self.obj = [np.asarray(t, np.float64) for t in targets]
        extent = max(np.ptp(t[:, :2], axis=0).max() for t in self.obj)
        self.poses = view_poses(len(self.obj), extent, self.cam, size, rng, tilt_deg, fill) if poses is None else np.asarray(poses, np.float64)
        noise_rng = np.random.default_rng(seed + 977)
        self.img = []
        for X, p in zip(self.obj, self.poses):
            px = cn.project(self.cam, p, X)
            self.img.append(px + noise * noise_rng.standard_normal(px.shape) if noise else px)

    def problem(self, free):
        return cn.make_problem(self.obj, self.img, free)

    def subset(self, views):
        s = object.__new__(Scene)
        s.size, s.cam = self.size, self.cam
        s.obj, s.img, s.poses = [self.obj[v] for v in views], [self.img[v] for v in views], self.poses[list(views)]
        return s


def perturbed_start(sc, free, seed=1, rel=2e-3, pose=2e-3):
    """the truth moved: free camera entries by up to rel (relative; a zero entry by rel absolute), poses by `pose` (rad, and relative
    to the distance) -- far enough for residuals of a few pixels, near enough for every lambda's step to exist"""
    rng = np.random.default_rng(seed)
    c = sc.cam.copy()
    for i in free:
        c[i] += rel * rng.uniform(-1, 1) * (abs(c[i]) if c[i] != 0.0 else 1.0)
    p = sc.poses.copy()
    p[:, :3] += pose * rng.uniform(-1, 1, p[:, :3].shape)
    p[:, 3:] += pose * rng.uniform(-1, 1, p[:, 3:].shape) * np.abs(p[:, 5:6])
    return c, p


def parity_scene(cam):
    """V = 12 views of a 9 x 6 grid (54 points a view)"""
    return Scene([grid(9, 6, 0.025)] * 12, cam, seed=3)


def smallest_scene():
    """V = 3, one 2 x 2 target of 4 points per view: with free = {fx, fy} 24 residuals against 20 unknowns"""
    return Scene([grid(2, 2, 0.1)] * 3, CAM5, seed=7)


TILE_COUNTS = (4, 63, 64, 65, 128, 129)


def tile_scene():
    """views of 4, 63, 64, 65, 128 and 129 points (the accumulation's tile is 64): random points of one 0.2 m square"""
    rng = np.random.default_rng(17)
    targets = []
    for n in TILE_COUNTS:
        xy = rng.uniform(-0.1, 0.1, (n, 2))
        xy[:4] = [[-0.1, -0.1], [0.1, -0.1], [0.1, 0.1], [-0.1, 0.1]]
        targets.append(np.concatenate([xy, np.zeros((n, 1))], axis=1))
    return Scene(targets, CAM5, seed=19)


def recovery_scene():
    """V = 8 views of a 6 x 5 grid, noise-free, the 5-coefficient camera"""
    return Scene([grid(6, 5, 0.04)] * 8, CAM5, seed=11)


N_CAL, N_HELD = 20, 8


def noisy_scene():
    """V = 20 (+ 8 held out) views of a 9 x 6 grid, sigma = 0.2 px"""
    return Scene([grid(9, 6, 0.025)] * (N_CAL + N_HELD), CAM5, seed=13, noise=0.2)


def fronto_scene():
    """every view parallel to the sensor: no tilt, roll and distance vary"""
    rng = np.random.default_rng(23)
    poses = np.array([[0.0, 0.0, rng.uniform(-0.5, 0.5), rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01), rng.uniform(0.25, 0.4)] for _ in range(5)])
    return Scene([grid(6, 5, 0.04)] * 5, np.concatenate([CAM5[:4], np.zeros(12)]), seed=23, poses=poses)


def nonplanar_scene():
    """V = 6 views of a 6 x 5 grid whose points are lifted out of the plane by up to 3 cm"""
    g = grid(6, 5, 0.04)
    g[:, 2] = 0.03 * np.sin(np.arange(len(g)) * 1.7)
    return Scene([g] * 6, CAM5, seed=29)


# ---- the end-to-end test: a flat tag board recorded with the camera that also films the body
E2E_SIZE = (1280, 720)
# a wide-angle lens: the body fills the middle 500 px of the frame only, and with a milder barrel (k1 = -0.28) the nominal camera's worst
# frame sits at 2.04 px, on the tracker's 2 px gate; with this one at 2.67 px (tests/test_camera_calib.py measures both)
E2E_CAM = np.array([1000.0, 1000.0, 640.0, 360.0, -0.5, 0.3, 8e-4, -6e-4, -0.1, 0, 0, 0, 0, 0, 0, 0])
E2E_BOARD_VIEWS = 15


def e2e_board():
    """4 x 3 tags of 30 mm at a pitch of 45 mm in the plane z = 0 -> the april_group dict"""
    tags = {}
    for j in range(3):
        for i in range(4):
            tags[str(4 * j + i)] = {"size": 0.03, "extrinsics": [float((i - 1.5) * 0.045), float((j - 1.0) * 0.045), 0.0, 0.0, 0.0, 0.0]}
    return {"tags": tags}


def e2e_board_recording(noise=0.05):
    """E2E_BOARD_VIEWS frames of the board under E2E_CAM (every tag in every frame, sigma = 0.05 px) -> (board, frames)"""
    from accurate_aprilgroup_tracking_amd import group_calib
    board = e2e_board()
    ids = sorted(int(t) for t in board["tags"])
    pts = group_calib.object_points(group_calib.group_to_poses(board, ids), [0.03] * len(ids))
    sc = Scene([pts] * E2E_BOARD_VIEWS, E2E_CAM, seed=31, noise=noise, size=E2E_SIZE, fill=0.45)
    frames = [[formats.make_detection(t, m.reshape(-1, 4, 2)[k]) for k, t in enumerate(ids)] for m in sc.img]
    return board, frames


def e2e_nominal_camera():
    """what a user without a calibration would write down: focal length = the image width, principal point at the centre, no distortion"""
    w, h = E2E_SIZE
    return np.array([[float(w), 0.0, w / 2.0], [0.0, float(w), h / 2.0], [0.0, 0.0, 1.0]]), np.zeros(5)


def e2e_body_clip():
    """the clip of the body (calib_scenes' end-to-end group and path) filmed with E2E_CAM"""
    import calib_scenes as cs
    K, dist = cn.split(E2E_CAM)
    assert np.array_equal(K, cs.synthetic.camera_matrix(*E2E_SIZE))
    sc = cs.Scene(12, 20, seed=13, dist=dist[:5], max_view_deg=60.0, max_polar_deg=60.0)
    assert (sc.visible.sum(axis=1) >= 2).all()
    return sc
