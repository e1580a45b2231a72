"""Independent numpy statement of the dense photometric + geometric pose refinement (TEST INFRASTRUCTURE).

Written from the SPECIFICATION block at the top of oracle/cv_dense.c, NOT from the C below it: float64 throughout, vectorised
over the samples, the projection and its 2 x 6 Jacobian from tests/pnp_numpy.project (0 / 4 / 5 / 8 / 12 / 14 coefficients, tilt
included), numpy.linalg for the 6 x 6 system.  It exists so that the oracle's loop -- which samples count at which iteration, the
damping, when the iteration stops, what the statistics say -- has a second implementation (tests/test_dense_edges.py).

    cost     E(p) = sum_j |project(obj_j; p) - img_j|^2 + photo_weight * sum_i (I~(project(X_i; p)) - T_i)^2
    sample   valid iff 1 <= floor(u) <= w - 3 and 1 <= floor(v) <= h - 3; I~ bilinear; gradient = bilinear interpolation of the
             central differences at the four integer neighbours
    solver   repeat `iters` times: A = J^T J, g = J^T r (photometric rows weighted by photo_weight); A_kk *= 1 + mu; A dx = g;
             p <- p - dx; stop when |dx| / (|p_before| + DBL_EPSILON) < FLT_EPSILON.  A not positive definite: the iteration
             counts, the pose stays, the loop ends.

refine() also returns what a test needs to know whether a scene is fit to compare two implementations on: how close any sample
came to a boundary of the validity window, the stop rule's ratio and cond(A) of every iteration.
"""
import numpy as np

import pnp_numpy

FLT_EPSILON = pnp_numpy.FLT_EPSILON
DBL_EPSILON = pnp_numpy.DBL_EPSILON


def central_differences(img):
    """-> (gx, gy) float64, same shape: (I(x+1, y) - I(x-1, y)) / 2 and (I(x, y+1) - I(x, y-1)) / 2; the outermost ring, which
    no valid sample touches, is left zero"""
    f = np.asarray(img, np.float64)
    gx, gy = np.zeros_like(f), np.zeros_like(f)
    gx[:, 1:-1] = (f[:, 2:] - f[:, :-2]) * 0.5
    gy[1:-1, :] = (f[2:, :] - f[:-2, :]) * 0.5
    return gx, gy


def valid_window(uv, w, h):
    """(n,) bool: 1 <= floor(u) <= w - 3 and 1 <= floor(v) <= h - 3 (false for a point that is not finite)"""
    with np.errstate(invalid="ignore"):
        x0, y0 = np.floor(uv[:, 0]), np.floor(uv[:, 1])
        return (x0 >= 1) & (x0 <= w - 3) & (y0 >= 1) & (y0 <= h - 3)


def bilinear(f, uv):
    """bilinear interpolation of the float64 image f at VALID points uv (n, 2)"""
    x0, y0 = np.floor(uv[:, 0]).astype(np.int64), np.floor(uv[:, 1]).astype(np.int64)
    a, b = uv[:, 0] - x0, uv[:, 1] - y0
    return (1 - a) * (1 - b) * f[y0, x0] + a * (1 - b) * f[y0, x0 + 1] + (1 - a) * b * f[y0 + 1, x0] + a * b * f[y0 + 1, x0 + 1]


def sample(img, uv):
    """-> (I, gx, gy, valid): intensity and gradient at uv (n, 2), zero where the sample is invalid"""
    f = np.asarray(img, np.float64)
    h, w = f.shape
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    ok = valid_window(uv, w, h)
    out = np.zeros((3, uv.shape[0]))
    if ok.any():
        gxi, gyi = central_differences(f)
        for q, src in enumerate((f, gxi, gyi)):
            out[q, ok] = bilinear(src, uv[ok])
    return out[0], out[1], out[2], ok


def window_margin(uv, w, h):
    """smallest distance of any finite u from 1 or w - 2, or v from 1 or h - 2: the places where a sample's validity flips"""
    uv = uv[np.isfinite(uv).all(axis=1)]
    if uv.shape[0] == 0:
        return np.inf
    du = np.minimum(np.abs(uv[:, 0] - 1.0), np.abs(uv[:, 0] - (w - 2.0)))
    dv = np.minimum(np.abs(uv[:, 1] - 1.0), np.abs(uv[:, 1] - (h - 2.0)))
    return float(min(du.min(), dv.min()))


def refine(img, model_xyz, model_t, obj, img_pts, mask, K, dist, rvec, tvec, iters=5, photo_weight=0.01, mu=1e-3):
    """-> (rvec (3,), tvec (3,), stats, diag).
    stats: photo_rms, geo_rms, valid, iters, used -- the residual statistics at the LAST linearisation point.
    diag: margin (smallest window_margin over all iterations), ratio (the stop rule's |dx| / (|p| + eps) of every iteration that
    solved), cond (cond(A) after damping, every iteration), solved (bool per iteration)."""
    f = np.asarray(img, np.float64)
    h, w = f.shape
    gxi, gyi = central_differences(f)
    K = np.asarray(K, np.float64).reshape(3, 3)
    X = np.asarray(model_xyz, np.float32).astype(np.float64).reshape(-1, 3)
    T = np.asarray(model_t, np.float32).astype(np.float64).reshape(-1)
    if obj is None:
        O = np.zeros((0, 3)); m2 = np.zeros((0, 2)); keep = np.zeros(0, bool)
    else:
        O = np.asarray(obj, np.float32).astype(np.float64).reshape(-1, 3)
        m2 = np.asarray(img_pts, np.float32).astype(np.float64).reshape(-1, 2)
        keep = np.ones(O.shape[0], bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    p = np.concatenate([np.asarray(rvec, np.float64).reshape(3), np.asarray(tvec, np.float64).reshape(3)])
    stats = dict(photo_rms=0.0, geo_rms=0.0, valid=0, iters=0, used=0)
    diag = dict(margin=np.inf, ratio=[], cond=[], solved=[])
    for it in range(int(iters)):
        A, g = np.zeros((6, 6)), np.zeros(6)
        e_geo, used = 0.0, int(keep.sum())
        if used:
            uv, J = pnp_numpy.project(O, p[:3], p[3:], K, dist, jacobian=True)
            e = (uv - m2)[keep].reshape(-1)
            J = J.reshape(-1, 2, 6)[keep].reshape(-1, 6)
            A += J.T @ J
            g += J.T @ e
            e_geo = float(e @ e)
        e_ph, valid = 0.0, 0
        if X.shape[0]:
            uv, J = pnp_numpy.project(X, p[:3], p[3:], K, dist, jacobian=True)
            diag["margin"] = min(diag["margin"], window_margin(uv, w, h))
            ok = valid_window(uv, w, h)
            valid = int(ok.sum())
            if valid:
                uvk, Ju, Jv = uv[ok], J[0::2][ok], J[1::2][ok]
                r = bilinear(f, uvk) - T[ok]
                Jr = bilinear(gxi, uvk)[:, None] * Ju + bilinear(gyi, uvk)[:, None] * Jv
                A += photo_weight * (Jr.T @ Jr)
                g += photo_weight * (Jr.T @ r)
                e_ph = float(r @ r)
        stats = dict(photo_rms=np.sqrt(e_ph / valid) if valid else 0.0, geo_rms=np.sqrt(e_geo / (2 * used)) if used else 0.0,
                     valid=valid, iters=it + 1, used=used)
        A[np.diag_indices(6)] *= 1.0 + mu
        with np.errstate(all="ignore"):
            diag["cond"].append(float(np.linalg.cond(A)) if np.isfinite(A).all() else np.inf)
        try:
            np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            diag["solved"].append(False)
            break
        diag["solved"].append(True)
        dx = np.linalg.solve(A, g)
        ratio = float(np.linalg.norm(dx) / (np.linalg.norm(p) + DBL_EPSILON))
        diag["ratio"].append(ratio)
        p = p - dx
        if ratio < FLT_EPSILON:
            break
    return p[:3].copy(), p[3:].copy(), stats, diag
