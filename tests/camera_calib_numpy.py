"""Independent numpy / scipy statement of the camera calibration (TEST INFRASTRUCTURE).

Written from the problem statement in include/agt_camcal.h, not from the kernels:
    unknowns   the camera vector c[16] = fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 (the entries of `free` only) and one pose
               p_v = (rvec, tvec) target -> camera per view
    residual   cv::projectPoints(X; p_v, c) - observed, two rows per point;   cost = 1/2 sum r^2
The projection and its pose Jacobian are tests/pnp_numpy.project (OpenCV's 3 x 9 dR/dr table); the camera block is written out here
from the projection's formulas.  The damped step is stated twice -- dense normal equations and a Schur complement over the view
blocks, both through numpy.linalg.solve -- and the minimisation is scipy.optimize.least_squares at tight tolerances.

A problem is a dict: obj (list of (n_v, 3)), img (list of (n_v, 2)), free (sorted list of camera entries).
Parameter order of the free vector: the free camera entries (ascending), then the views (6 each).
"""
import numpy as np
import scipy.optimize

import pnp_numpy

NCAM = 16


def make_problem(obj, img, free):
    free = sorted(int(i) for i in (free if not isinstance(free, (int, np.integer)) else [i for i in range(NCAM) if int(free) >> i & 1]))
    return dict(obj=[np.asarray(o, np.float64).reshape(-1, 3) for o in obj], img=[np.asarray(m, np.float64).reshape(-1, 2) for m in img], free=free)


def mask_of(prob):
    return sum(1 << i for i in prob["free"])


def split(c):
    """c[16] -> (K (3, 3), dist (12,))"""
    c = np.asarray(c, np.float64)
    return np.array([[c[0], 0.0, c[2]], [0.0, c[1], c[3]], [0.0, 0.0, 1.0]]), c[4:16].copy()


def project(c, pose, X):
    K, d = split(c)
    return pnp_numpy.project(X, pose[:3], pose[3:], K, d)


def residuals(prob, c, poses):
    """(N, 2): projected - observed, views and points in the problem's order"""
    return np.concatenate([project(c, poses[v], X) - prob["img"][v] for v, X in enumerate(prob["obj"])])


def camera_block(c, pose, X):
    """(2n, 16): d(u, v) / d c at the points X of a view.  With (x, y) the normalised point, r2 = x^2 + y^2,
    num = 1 + k1 r2 + k2 r4 + k3 r6, den = 1 + k4 r2 + k5 r4 + k6 r6:
        xd = x num / den + 2 p1 x y + p2 (r2 + 2 x^2) + s1 r2 + s2 r4,   u = fx xd + cx
        yd = y num / den + p1 (r2 + 2 y^2) + 2 p2 x y + s3 r2 + s4 r4,   v = fy yd + cy"""
    c = np.asarray(c, np.float64)
    fx, fy = c[0], c[1]
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = c[4:16]
    R, _ = pnp_numpy.rodrigues(pose[:3])
    Yc = np.asarray(X, np.float64).reshape(-1, 3) @ R.T + pose[3:]
    x, y = Yc[:, 0] / Yc[:, 2], Yc[:, 1] / Yc[:, 2]
    r2 = x * x + y * y
    r4, r6 = r2 ** 2, r2 ** 3
    num = 1 + k1 * r2 + k2 * r4 + k3 * r6
    den = 1 + k4 * r2 + k5 * r4 + k6 * r6
    xd = x * num / den + 2 * p1 * x * y + p2 * (r2 + 2 * x * x) + s1 * r2 + s2 * r4
    yd = y * num / den + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y + s3 * r2 + s4 * r4
    n = len(x)
    J = np.zeros((n, 2, NCAM))
    J[:, 0, 0] = xd; J[:, 0, 2] = 1.0
    J[:, 1, 1] = yd; J[:, 1, 3] = 1.0
    for col, pw in ((4, r2), (5, r4), (8, r6)):                    # numerator
        J[:, 0, col] = fx * x * pw / den; J[:, 1, col] = fy * y * pw / den
    for col, pw in ((9, r2), (10, r4), (11, r6)):                  # denominator
        J[:, 0, col] = -fx * x * num * pw / den ** 2; J[:, 1, col] = -fy * y * num * pw / den ** 2
    J[:, 0, 6] = fx * 2 * x * y; J[:, 1, 6] = fy * (r2 + 2 * y * y)
    J[:, 0, 7] = fx * (r2 + 2 * x * x); J[:, 1, 7] = fy * 2 * x * y
    J[:, 0, 12] = fx * r2; J[:, 0, 13] = fx * r4
    J[:, 1, 14] = fy * r2; J[:, 1, 15] = fy * r4
    return J.reshape(2 * n, NCAM)


def blocks(prob, c, poses):
    """per view: residual (2n,), J_c (2n, 16), J_v (2n, 6)"""
    K, d = split(c)
    out = []
    for v, X in enumerate(prob["obj"]):
        img, Jv = pnp_numpy.project(X, poses[v, :3], poses[v, 3:], K, d, jacobian=True)
        out.append(((img - prob["img"][v]).reshape(-1), camera_block(c, poses[v], X), Jv))
    return out


def jacobian(prob, c, poses):
    """-> (r (2N,), J (2N, n_free + 6 V)) dense"""
    free = prob["free"]; nf = len(free); V = len(prob["obj"])
    bl = blocks(prob, c, poses)
    N2 = sum(len(b[0]) for b in bl)
    J = np.zeros((N2, nf + 6 * V)); r = np.zeros(N2)
    row = 0
    for v, (rv, Jc, Jv) in enumerate(bl):
        m = len(rv)
        r[row:row + m] = rv
        J[row:row + m, :nf] = Jc[:, free]
        J[row:row + m, nf + 6 * v:nf + 6 * v + 6] = Jv
        row += m
    return r, J


def _unpack(prob, d):
    nf = len(prob["free"])
    dc = np.zeros(NCAM)
    dc[prob["free"]] = d[:nf]
    return dc, d[nf:].reshape(-1, 6).copy()


def dense_step(prob, c, poses, lam):
    """(J^T J + lam diag(J^T J)) d = -J^T r, solved densely -> (d_camera (16,), d_views (V, 6))"""
    r, J = jacobian(prob, c, poses)
    H = J.T @ J
    return _unpack(prob, np.linalg.solve(H + lam * np.diag(np.diag(H)), -(J.T @ r)))


def schur_step(prob, c, poses, lam):
    """the same step with the view blocks eliminated first"""
    free = prob["free"]; nf = len(free)
    S = np.zeros((nf, nf)); rhs = np.zeros(nf); A = np.zeros((nf, nf))
    Y, x = [], []
    for rv, Jc, Jv in blocks(prob, c, poses):
        Jc = Jc[:, free]
        U = Jv.T @ Jv
        Ud = U + lam * np.diag(np.diag(U))
        B = Jc.T @ Jv
        A += Jc.T @ Jc
        rhs += Jc.T @ rv
        Y.append(np.linalg.solve(Ud, B.T)); x.append(np.linalg.solve(Ud, Jv.T @ rv))
        S -= B @ Y[-1]
        rhs -= B @ x[-1]
    S += A + lam * np.diag(np.diag(A))
    d = np.linalg.solve(S, -rhs)
    dc = np.zeros(NCAM); dc[free] = d
    return dc, np.array([-xv - Yv @ d for Yv, xv in zip(Y, x)])


def step_difference(a, b):
    """relative difference of two steps (d_camera, d_views), against the norm of the second"""
    va = np.concatenate([a[0].ravel(), a[1].ravel()]); vb = np.concatenate([b[0].ravel(), b[1].ravel()])
    return float(np.linalg.norm(va - vb) / np.linalg.norm(vb))


def scaled_condition(prob, c, poses):
    """condition number of J with its columns scaled to unit length"""
    _, J = jacobian(prob, c, poses)
    return float(np.linalg.cond(J / np.linalg.norm(J, axis=0)))


def solve(prob, c, poses, max_nfev=400):
    """scipy.optimize.least_squares (MINPACK Levenberg-Marquardt, analytic Jacobian) at the tightest tolerances it accepts
    -> (c, poses, cost, rms per residual)"""
    free = prob["free"]; nf = len(free)
    c0 = np.array(c, np.float64); V = len(prob["obj"])

    def unpack(x):
        cc = c0.copy(); cc[free] = x[:nf]
        return cc, x[nf:].reshape(V, 6)

    x0 = np.concatenate([c0[free], np.asarray(poses, np.float64).ravel()])
    eps = 4 * np.finfo(np.float64).eps
    res = scipy.optimize.least_squares(lambda x: residuals(prob, *unpack(x)).ravel(), x0, jac=lambda x: jacobian(prob, *unpack(x))[1],
                                       method="lm", x_scale="jac", ftol=eps, xtol=eps, gtol=eps, max_nfev=max_nfev)
    cc, pp = unpack(res.x)
    co = 0.5 * float(res.fun @ res.fun)
    return cc, pp.copy(), co, float(np.sqrt(2.0 * co / res.fun.size))
