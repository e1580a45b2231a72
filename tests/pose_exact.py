"""Exact statement of the pose operations every kernel shares (TEST INFRASTRUCTURE): mpmath at 100 digits.

Written from the mathematics, not from csrc/agt_device.h and not from OpenCV's code:
    R(r)      = exp([r]x) = I + sin(t)/t [r]x + 2 sin^2(t/2)/t^2 [r]x^2,  t = |r|        (no 1 - cos: nothing cancels)
    pixel     = K distort(tilt)((R X + t) / z): the 14-coefficient model of the calib3d documentation (rational radial, tangential,
                thin prism, tilted sensor); fewer coefficients = the rest zero
    Jacobian  = d pixel / d (r, t) by central differences with a step of 1e-30 IN multiprecision: truncation ~1e-60 of the third
                derivative, rounding ~1e-70 -- exact to far more than the 17 digits the results are rounded to
    log(R)    = the rotation vector of a rotation matrix, |log| <= pi
    predict   = the constant-velocity extrapolation of agt_predict_flow: D = R1 R2^T, Rp = D R1, tp = D (t1 - t2) + t1
Inputs are float64 (converted exactly); outputs are mpmath numbers until `f64` rounds them ONCE.  The module also holds the ladders
of rotations and the scenes that tests/golden/make_pose_range_fixture.py tabulates into tests/golden/pose_range.npz: the GPU tests
read only that file (mpmath need not exist where they run).
"""
import math

import mpmath as mp
import numpy as np

from pose_range_scenes import rotation as rotation_f64

mp.mp.dps = 100
H = mp.mpf(10) ** -30
EPS = float(np.finfo(np.float64).eps)


def _v(x):
    return [x_ if isinstance(x_, mp.mpf) else mp.mpf(float(x_)) for x_ in np.asarray(x, object).reshape(-1)]


def f64(a):
    """round once to float64"""
    return np.array([float(x) for x in np.asarray(a, object).reshape(-1)]).reshape(np.shape(a))


def skew(r):
    return mp.matrix([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])


def rotation(rvec):
    r = _v(rvec)
    t2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
    if t2 == 0:
        return mp.eye(3)
    t = mp.sqrt(t2)
    Kx = skew(r)
    return mp.eye(3) + (mp.sin(t) / t) * Kx + (2 * mp.sin(t / 2) ** 2 / t2) * (Kx * Kx)


def tilt(tau_x, tau_y):
    """as tests/pnp_numpy.tilt_matrix: [[R22, 0, -R02], [0, R22, -R12], [0, 0, 1]] R with R = R_y(tau_y) R_x(tau_x)"""
    cx, sx, cy, sy = mp.cos(tau_x), mp.sin(tau_x), mp.cos(tau_y), mp.sin(tau_y)
    Rx = mp.matrix([[1, 0, 0], [0, cx, sx], [0, -sx, cx]])
    Ry = mp.matrix([[cy, 0, -sy], [0, 1, 0], [sy, 0, cy]])
    R = Ry * Rx
    return mp.matrix([[R[2, 2], 0, -R[0, 2]], [0, R[2, 2], -R[1, 2]], [0, 0, 1]]) * R


class Camera:
    """K (3, 3) float64; dist: None or 4, 5, 8, 12 or 14 float64 coefficients (k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 tau_x tau_y)"""

    def __init__(self, K, dist=None):
        K = np.asarray(K, np.float64)
        self.f = (mp.mpf(K[0, 0]), mp.mpf(K[1, 1]))
        self.c = (mp.mpf(K[0, 2]), mp.mpf(K[1, 2]))
        d = np.zeros(14)
        if dist is not None:
            dd = np.asarray(dist, np.float64).reshape(-1)
            assert dd.size in (4, 5, 8, 12, 14)
            d[:dd.size] = dd
        self.k = [mp.mpf(x) for x in d]
        self.T = tilt(self.k[12], self.k[13]) if (d[12:] != 0).any() else None

    def pixel(self, Y):
        """camera-frame point -> (u, v)"""
        k = self.k
        x, y = Y[0] / Y[2], Y[1] / Y[2]
        r2 = x * x + y * y
        radial = (1 + r2 * (k[0] + r2 * (k[1] + r2 * k[4]))) / (1 + r2 * (k[5] + r2 * (k[6] + r2 * k[7])))
        xd = x * radial + 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + r2 * (k[8] + r2 * k[9])
        yd = y * radial + k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + r2 * (k[10] + r2 * k[11])
        if self.T is not None:
            T = self.T
            w = T[2, 0] * xd + T[2, 1] * yd + T[2, 2]
            xd, yd = (T[0, 0] * xd + T[0, 1] * yd + T[0, 2]) / w, (T[1, 0] * xd + T[1, 1] * yd + T[1, 2]) / w
        return self.f[0] * xd + self.c[0], self.f[1] * yd + self.c[1]


def _camera_points(obj, rvec, tvec):
    R, t = rotation(rvec), _v(tvec)
    out = []
    for X in np.asarray(obj, object).reshape(-1, 3):
        X = _v(X)
        out.append([R[i, 0] * X[0] + R[i, 1] * X[1] + R[i, 2] * X[2] + t[i] for i in range(3)])
    return out


def project(obj, rvec, tvec, cams, jacobian=False):
    """obj (n, 3), one pose, a list of cameras -> per camera (pixels (n, 2) [, J (n, 2, 6) = d(u, v)/d(rvec, tvec)]) of mpmath
    numbers.  The seven rotations of the differences are formed once and shared by the cameras."""
    r, t = _v(rvec), _v(tvec)
    n = len(np.asarray(obj, object).reshape(-1, 3))
    base = _camera_points(obj, r, t)
    moved = []
    if jacobian:
        for j in range(6):
            pair = []
            for sgn in (1, -1):
                p = r + t
                p[j] = p[j] + sgn * H
                pair.append(_camera_points(obj, p[:3], p[3:]))
            moved.append(pair)
    out = []
    for cam in cams:
        px = np.empty((n, 2), object)
        for i in range(n):
            px[i] = cam.pixel(base[i])
        if not jacobian:
            out.append(px)
            continue
        J = np.empty((n, 2, 6), object)
        for j in range(6):
            for i in range(n):
                a, b = cam.pixel(moved[j][0][i]), cam.pixel(moved[j][1][i])
                J[i, 0, j] = (a[0] - b[0]) / (2 * H)
                J[i, 1, j] = (a[1] - b[1]) / (2 * H)
        out.append((px, J))
    return out


def log_rotation(R):
    """rotation matrix (mpmath) -> rotation vector, |.| <= pi; at pi exactly the axis with the largest component positive"""
    v = [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]
    s = mp.sqrt(v[0] ** 2 + v[1] ** 2 + v[2] ** 2) / 2
    c = (R[0, 0] + R[1, 1] + R[2, 2] - 1) / 2
    if s == 0:
        if c > 0:
            return [mp.mpf(0)] * 3
        i = max(range(3), key=lambda q: R[q, q])
        col = [(R[q, i] + (1 if q == i else 0)) / 2 for q in range(3)]          # column i of (R + I) / 2 = a a_i
        nrm = mp.sqrt(col[0] ** 2 + col[1] ** 2 + col[2] ** 2)
        return [mp.pi * x / nrm for x in col]
    theta = mp.atan2(s, c)
    return [x * theta / (2 * s) for x in v]


def predict(older, newer):
    """two poses (rvec | tvec, float64) -> (Rp 3 x 3, tp 3) of the constant-velocity extrapolation"""
    R2, R1 = rotation(older[:3]), rotation(newer[:3])
    D = R1 * R2.T
    d = mp.matrix([mp.mpf(float(a)) - mp.mpf(float(b)) for a, b in zip(newer[3:], older[3:])])
    tp = D * d + mp.matrix(_v(newer[3:]))
    return D * R1, [tp[i] for i in range(3)]


# ------------------------------------------------------------------------------------------------------------------ ladders and scenes
AXES = {"general": np.array([0.6, -0.48, 0.64]), "+x": np.array([1.0, 0.0, 0.0]), "-y": np.array([0.0, -1.0, 0.0])}
# 1e-2 is the double the kernel compares with: itself (closed form) and its predecessor (series)
ANGLES = [0.0, 1e-17, 3e-16, 1e-12, 1e-9, 1e-8, 1e-6, 1e-4, 5e-3, float(np.nextafter(1e-2, 0.0)), 1e-2, 0.37, math.pi / 2,
          3.1, math.pi - 1e-6, math.pi, math.pi + 1e-3, 6.2, 7.0, 2.0 ** 20 - 0.5, 2.0 ** 20 + 0.5]
WIDTH, HEIGHT, FOCAL = 1280, 720, 900.0
K = np.array([[FOCAL, 0.0, WIDTH / 2.0], [0.0, FOCAL, HEIGHT / 2.0], [0.0, 0.0, 1.0]])
TVEC = np.array([0.01, -0.02, 0.4])
MILD_DIST = np.array([0.05, -0.1, 1e-3, -1e-3, 0.02])                     # synthetic.MILD_DIST (test_pose_exact asserts it)
TILT14 = np.array([0.05, -0.1, 1e-3, -1e-3, 0.02, 0.01, -0.02, 0.005, 1e-3, -5e-4, 5e-4, 1e-3, 0.02, -0.015])   # calib_scenes.TILT14
CAMERAS = {"pinhole": None, "mild": MILD_DIST, "tilt14": TILT14}
# the sixth point is placed per rung so that it lands 10 px inside the image corner, where the distortion terms are largest:
# camera-frame direction (x / z, y / z) = (0.70, -0.39) against the border's (0.711, -0.4)
BORDER_RAY = np.array([0.70, -0.39, 1.0]) * 0.4


def ladder():
    """-> (names, thetas (B,), rvecs (B, 3)): every angle about every axis, rvec = theta * axis in float64"""
    names, th, rv = [], [], []
    for an, a in AXES.items():
        for t in ANGLES:
            names.append("%s %.17g" % (an, t)); th.append(t); rv.append(t * a)
    return names, np.array(th), np.array(rv)


def ladder_points(rvecs):
    """(B, 6, 3): the corners of a 20 mm tag, the origin, and the border point of each rung"""
    h = 0.01
    fixed = np.array([[-h, -h, 0.0], [-h, h, 0.0], [h, h, 0.0], [h, -h, 0.0], [0.0, 0.0, 0.0]])
    out = np.empty((len(rvecs), 6, 3))
    for b, r in enumerate(rvecs):
        out[b, :5] = fixed
        # (float64, rounded to the micrometre so that the last bits of a platform's sin and cos cannot reach the table: it only places the point)
        out[b, 5] = np.round(rotation_f64(r).T @ (BORDER_RAY - TVEC), 6)
    return out


# agt_rodrigues_inv through agt_predict_flow: older = (0, t2), newer = (phi / 2 * a, t1) -> the predicted rotation is exp(phi a)
INV_AXES9 = {"+x": [1.0, 0, 0], "-x": [-1.0, 0, 0], "+y": [0, 1.0, 0], "-y": [0, -1.0, 0], "+z": [0, 0, 1.0], "-z": [0, 0, -1.0],
             "general": [0.6, -0.48, 0.64], "-general": [-0.6, 0.48, -0.64], "x smallest": [2.0 / 7, 3.0 / 7, -6.0 / 7]}
INV_T2, INV_T1 = np.array([0.012, -0.018, 0.41]), np.array([0.01, -0.02, 0.4])
SIN_RULE = 1e-5          # the threshold on |sin theta| in agt_rodrigues_inv


def inverse_ladder():
    """-> (names, kinds, phis, older (B, 6), newer (B, 6)); kind: 'zero' (the zero rule), 'pi' (the theta = pi branch), 'generic'"""
    rows = [("general", 0.0), ("general", 5e-6), ("general", 2e-5), ("general", 1e-3), ("general", 1.0), ("general", math.pi - 1e-3),
            ("general", math.pi - 2e-5)]
    rows += [(a, p) for p in (math.pi - 5e-6, math.pi) for a in INV_AXES9]
    rows.append(("general", math.pi + 1e-3))
    names, kinds, phis, older, newer = [], [], [], [], []
    for an, phi in rows:
        a = np.array(INV_AXES9[an], np.float64)
        s, c = abs(math.sin(phi)), math.cos(phi)
        # a factor of two from the threshold on either side (sin(2e-5) is 2e-5 less 7e-11 of itself: the factor is taken to 1e-9)
        assert s <= SIN_RULE / 2 or s >= SIN_RULE * 2 * (1 - 1e-9), (an, phi)
        kinds.append("generic" if s > SIN_RULE else ("zero" if c > 0 else "pi"))
        names.append("%s %.17g" % (an, phi)); phis.append(phi)
        older.append(np.concatenate([np.zeros(3), INV_T2])); newer.append(np.concatenate([phi / 2 * a, INV_T1]))
    return names, kinds, np.array(phis), np.array(older), np.array(newer)


# solvePnP with a guess: 12 non-coplanar points, truth rotations about the general axis, the guess 0.02 rad and 3 mm off
PNP_ANGLES = [0.0, 1e-9, 5e-3, 1e-2, math.pi / 2, math.pi - 1e-6, math.pi, math.pi + 1e-3, 7.0]


def pnp_scene():
    """-> (obj (12, 3), truth (9, 6), guess (9, 6))"""
    rng = np.random.default_rng(21)
    obj = rng.uniform(-0.04, 0.04, (12, 3))
    truth = np.array([np.concatenate([t * AXES["general"], TVEC]) for t in PNP_ANGLES])
    guess = truth + np.array([0.02 / math.sqrt(3.0)] * 3 + [0.003 / math.sqrt(3.0)] * 3) * np.array([1, -1, 1, -1, 1, 1])
    return obj, truth, guess
