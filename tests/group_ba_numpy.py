"""Independent numpy / scipy statement of the AprilGroup bundle adjustment (TEST INFRASTRUCTURE).

Written from the problem statement in include/agt_calib.h, not from the kernels:
    unknowns   p_f = (rvec, tvec) body -> camera per frame, q_t = (rvec, tvec) tag -> body per tag, the anchor tag fixed
    corner k of tag t, r = size / 2: (-r,-r,0), (-r,r,0), (r,r,0), (r,-r,0);   X = R(q_t.r) c_k + q_t.t
    pixel = cv::projectPoints(X; p_f, camera);   residual = projected - observed (two rows per corner);   cost = 1/2 sum r^2
The projection and its Jacobian are tests/pnp_numpy.project (OpenCV's 3 x 9 dR/dr table, 14 coefficients with tilt); the tag block
follows by the chain rule through the same table.  The damped step is stated twice -- dense normal equations and a Schur complement
over the frame blocks, both through numpy.linalg.solve -- and the minimisation is scipy.optimize.least_squares at tight tolerances.

A problem is a dict: K (3,3), dist (k,) or None, sizes (T,), anchor, F, obs_frame (n,), obs_tag (n,), corners (n,4,2).
Parameter order of the free vector: the frames that have observations (6 each, ascending), then the tags but the anchor (6 each).
"""
import numpy as np
import scipy.optimize

import pnp_numpy


def corners3d(size):
    r = size / 2.0
    return np.array([[-r, -r, 0.0], [-r, r, 0.0], [r, r, 0.0], [r, -r, 0.0]])


def make_problem(K, dist, sizes, anchor, F, obs_frame, obs_tag, corners):
    return dict(K=np.asarray(K, np.float64).reshape(3, 3), dist=None if dist is None else np.asarray(dist, np.float64).reshape(-1),
                sizes=np.asarray(sizes, np.float64), anchor=int(anchor), F=int(F), obs_frame=np.asarray(obs_frame, np.int64),
                obs_tag=np.asarray(obs_tag, np.int64), corners=np.asarray(corners, np.float64).reshape(-1, 4, 2))


def _body_points(q, size):
    R, _ = pnp_numpy.rodrigues(q[:3])
    return corners3d(size) @ R.T + q[3:]


def residuals(prob, tag_poses, frame_poses):
    """(n, 8): projected - observed, (x, y) of corners 0..3, in the problem's observation order"""
    out = np.zeros((len(prob["obs_tag"]), 8))
    for i, (f, t) in enumerate(zip(prob["obs_frame"], prob["obs_tag"])):
        X = _body_points(tag_poses[t], prob["sizes"][t])
        out[i] = (pnp_numpy.project(X, frame_poses[f, :3], frame_poses[f, 3:], prob["K"], prob["dist"]) - prob["corners"][i]).reshape(8)
    return out


def cost(prob, tag_poses, frame_poses):
    r = residuals(prob, tag_poses, frame_poses)
    return 0.5 * float((r * r).sum())


def blocks(prob, tag_poses, frame_poses):
    """per observation: residual (8,), J_f (8, 6) w.r.t. the frame pose, J_t (8, 6) w.r.t. the tag pose"""
    out = []
    for i, (f, t) in enumerate(zip(prob["obs_frame"], prob["obs_tag"])):
        q = tag_poses[t]
        Rt, dRt = pnp_numpy.rodrigues(q[:3])
        c = corners3d(prob["sizes"][t])
        X = c @ Rt.T + q[3:]
        img, Jf = pnp_numpy.project(X, frame_poses[f, :3], frame_poses[f, 3:], prob["K"], prob["dist"], jacobian=True)
        Rf, _ = pnp_numpy.rodrigues(frame_poses[f, :3])
        Jt = np.zeros((8, 6))
        for k in range(4):
            dpdX = Jf[2 * k:2 * k + 2, 3:6] @ Rf                       # d pixel / d Y = the translation block; Y = R_f X + t_f
            for j in range(3):
                Jt[2 * k:2 * k + 2, j] = dpdX @ (dRt[j].reshape(3, 3) @ c[k])
            Jt[2 * k:2 * k + 2, 3:6] = dpdX
        out.append(((img - prob["corners"][i]).reshape(8), Jf, Jt))
    return out


def layout(prob):
    """-> (frame_col {f: first column}, tag_col {t: first column}, n_free)"""
    used = sorted(set(int(f) for f in prob["obs_frame"]))
    frame_col = {f: 6 * i for i, f in enumerate(used)}
    tags = [t for t in range(len(prob["sizes"])) if t != prob["anchor"]]
    tag_col = {t: 6 * len(used) + 6 * i for i, t in enumerate(tags)}
    return frame_col, tag_col, 6 * (len(used) + len(tags))


def jacobian(prob, tag_poses, frame_poses):
    """-> (r (8n,), J (8n, n_free)) dense"""
    fc, tc, m = layout(prob)
    n = len(prob["obs_tag"])
    J = np.zeros((8 * n, m)); r = np.zeros(8 * n)
    for i, (ri, Jf, Jt) in enumerate(blocks(prob, tag_poses, frame_poses)):
        f, t = int(prob["obs_frame"][i]), int(prob["obs_tag"][i])
        r[8 * i:8 * i + 8] = ri
        J[8 * i:8 * i + 8, fc[f]:fc[f] + 6] = Jf
        if t != prob["anchor"]:
            J[8 * i:8 * i + 8, tc[t]:tc[t] + 6] = Jt
    return r, J


def _unpack(prob, d):
    fc, tc, _ = layout(prob)
    d_tags = np.zeros((len(prob["sizes"]), 6)); d_frames = np.zeros((prob["F"], 6))
    for f, c in fc.items():
        d_frames[f] = d[c:c + 6]
    for t, c in tc.items():
        d_tags[t] = d[c:c + 6]
    return d_tags, d_frames


def dense_step(prob, tag_poses, frame_poses, lam):
    """(J^T J + lam diag(J^T J)) d = -J^T r, solved densely -> (d_tags (T,6), d_frames (F,6))"""
    r, J = jacobian(prob, tag_poses, frame_poses)
    H = J.T @ J
    A = H + lam * np.diag(np.diag(H))
    return _unpack(prob, np.linalg.solve(A, -(J.T @ r)))


def schur_step(prob, tag_poses, frame_poses, lam):
    """the same step with the frame blocks eliminated first"""
    T, a = len(prob["sizes"]), prob["anchor"]
    bl = blocks(prob, tag_poses, frame_poses)
    U, gf, V, gt, W = {}, {}, np.zeros((T, 6, 6)), np.zeros((T, 6)), {}
    for i, (r, Jf, Jt) in enumerate(bl):
        f, t = int(prob["obs_frame"][i]), int(prob["obs_tag"][i])
        U[f] = U.get(f, 0) + Jf.T @ Jf
        gf[f] = gf.get(f, 0) + Jf.T @ r
        V[t] += Jt.T @ Jt; gt[t] += Jt.T @ r
        W[(f, t)] = Jf.T @ Jt
    free = [t for t in range(T) if t != a]
    col = {t: 6 * i for i, t in enumerate(free)}
    S = np.zeros((6 * len(free), 6 * len(free))); rhs = np.zeros(6 * len(free))
    Y, x = {}, {}
    for t in free:
        S[col[t]:col[t] + 6, col[t]:col[t] + 6] = V[t] + lam * np.diag(np.diag(V[t]))
        rhs[col[t]:col[t] + 6] = gt[t]
    for f in U:
        A = U[f] + lam * np.diag(np.diag(U[f]))
        x[f] = np.linalg.solve(A, gf[f])
        seen = [t for t in free if (f, t) in W]
        for t in seen:
            Y[(f, t)] = np.linalg.solve(A, W[(f, t)])
        for t1 in seen:
            rhs[col[t1]:col[t1] + 6] -= W[(f, t1)].T @ x[f]
            for t2 in seen:
                S[col[t1]:col[t1] + 6, col[t2]:col[t2] + 6] -= W[(f, t1)].T @ Y[(f, t2)]
    dt = np.linalg.solve(S, -rhs) if len(free) else np.zeros(0)
    d_tags = np.zeros((T, 6)); d_frames = np.zeros((prob["F"], 6))
    for t in free:
        d_tags[t] = dt[col[t]:col[t] + 6]
    for f in U:
        d = -x[f]
        for t in free:
            if (f, t) in Y:
                d = d - Y[(f, t)] @ d_tags[t]
        d_frames[f] = d
    return d_tags, d_frames


def step_difference(a, b):
    """relative difference of two steps (d_tags, d_frames), against the norm of the second"""
    va = np.concatenate([a[0].ravel(), a[1].ravel()]); vb = np.concatenate([b[0].ravel(), b[1].ravel()])
    return float(np.linalg.norm(va - vb) / np.linalg.norm(vb))


def solve(prob, tag_poses, frame_poses, max_nfev=400):
    """scipy.optimize.least_squares (MINPACK Levenberg-Marquardt, analytic Jacobian) at the tightest tolerances it accepts
    -> (tag_poses, frame_poses, cost, rms)"""
    fc, tc, m = layout(prob)
    tag0 = np.array(tag_poses, np.float64); frame0 = np.array(frame_poses, np.float64)

    def unpack(x):
        tp, fp = tag0.copy(), frame0.copy()
        for f, c in fc.items():
            fp[f] = x[c:c + 6]
        for t, c in tc.items():
            tp[t] = x[c:c + 6]
        return tp, fp

    x0 = np.zeros(m)
    for f, c in fc.items():
        x0[c:c + 6] = frame0[f]
    for t, c in tc.items():
        x0[c:c + 6] = tag0[t]
    eps = 4 * np.finfo(np.float64).eps
    res = scipy.optimize.least_squares(lambda x: residuals(prob, *unpack(x)).ravel(), x0, jac=lambda x: jacobian(prob, *unpack(x))[1],
                                       method="lm", ftol=eps, xtol=eps, gtol=eps, max_nfev=max_nfev)
    tp, fp = unpack(res.x)
    c = 0.5 * float(res.fun @ res.fun)
    return tp, fp, c, float(np.sqrt(2.0 * c / res.fun.size))
