"""Independent numpy statement of the dense-model accumulation of include/agt_model.h (TEST INFRASTRUCTURE).

Written from the rule in the header: float64 throughout, vectorised over the samples, the projection from tests/pnp_numpy.project
(0 / 4 / 5 / 8 / 12 / 14 coefficients, tilt included), the validity window and the bilinear sample from tests/dense_numpy.  The frames
are walked in order and every sample's sums grow by one term per frame (a sample without an observation adds an exact 0.0), so the
sums are the rule's, in the rule's order.

A pass also returns how close any observation came to one of the rule's decisions -- the cos threshold, the window edges, the clip
gate: a scene in which one of them is nearly a tie cannot be used to compare two implementations.
"""
import numpy as np

import dense_numpy
import pnp_numpy


class Problem:
    def __init__(self, K, dist, width, height, tag_corners, model_xyz, sample_tag, max_view_deg=60.0, facing=1):
        self.K = np.asarray(K, np.float64).reshape(3, 3)
        self.dist = None if dist is None else np.asarray(dist, np.float64).reshape(-1)
        self.w, self.h = int(width), int(height)
        self.corners = np.asarray(tag_corners, np.float32).astype(np.float64).reshape(-1, 4, 3)
        self.X = np.asarray(model_xyz, np.float32).astype(np.float64).reshape(-1, 3)
        self.tag = np.asarray(sample_tag, np.int64).reshape(-1)
        self.max_view_deg, self.facing = float(max_view_deg), int(facing)
        self.M, self.T = self.X.shape[0], self.corners.shape[0]


def cos_threshold(max_view_deg):
    return 0.0 if max_view_deg == 90.0 else float(np.cos(np.deg2rad(max_view_deg)))


def tag_visibility(prob, pose):
    """-> (visible (T,) bool, cos (T,)) by the rule of agt_tracker_visibility"""
    R, _ = pnp_numpy.rodrigues(pose[:3])
    p = prob.corners
    c_o = (((p[:, 0] + p[:, 1]) + p[:, 2]) + p[:, 3]) * 0.25
    n_o = prob.facing * np.cross(p[:, 3] - p[:, 0], p[:, 1] - p[:, 0])
    c_c = c_o @ R.T + np.asarray(pose[3:], np.float64)
    n_c = n_o @ R.T
    with np.errstate(invalid="ignore", divide="ignore"):
        cs = -(n_c * c_c).sum(axis=1) / (np.sqrt((n_c * n_c).sum(axis=1)) * np.sqrt((c_c * c_c).sum(axis=1)))
        vis = (c_c[:, 2] > 0.0) & (cs > cos_threshold(prob.max_view_deg))
    return vis, cs


def observe(prob, frame, pose):
    """one frame -> (exists (M,) bool, I (M,) f64 (0 where there is no observation), cos margin, window margin)"""
    pose = np.asarray(pose, np.float64).reshape(6)
    vis, cs = tag_visibility(prob, pose)
    cos_margin = float(np.abs(cs - cos_threshold(prob.max_view_deg)).min())
    R, _ = pnp_numpy.rodrigues(pose[:3])
    z = (prob.X @ R.T + pose[3:])[:, 2]
    uv = pnp_numpy.project(prob.X, pose[:3], pose[3:], prob.K, prob.dist)
    cand = vis[prob.tag] & (z > 0.0)
    win_margin = dense_numpy.window_margin(uv[cand], prob.w, prob.h) if cand.any() else np.inf
    ok = cand & dense_numpy.valid_window(uv, prob.w, prob.h)
    I = np.zeros(prob.M)
    if ok.any():
        I[ok] = dense_numpy.bilinear(np.asarray(frame, np.float64), uv[ok])
    return ok, I, cos_margin, win_margin


def reference_of(result):
    """(n, mean_r, std_r) of a finished pass, as the clipped pass uses them"""
    n = result["n"]
    nn = np.where(n > 0, n, 1).astype(np.float64)
    mean = result["S"] / nn
    std = np.sqrt(np.maximum(result["S2"] / nn - mean * mean, 0.0))
    return n, mean, std


def run_pass(prob, frames, poses, use=None, ref=None, clip_sigma=0.0, sigma_floor=0.0):
    """-> dict(n, S, S2, rejected, frame_obs, margins=dict(cos, window, clip)); ref: the result of the previous pass (clipped pass)"""
    poses = np.asarray(poses, np.float64).reshape(-1, 6)
    F = poses.shape[0]
    n, rej = np.zeros(prob.M, np.int64), np.zeros(prob.M, np.int64)
    S, S2 = np.zeros(prob.M), np.zeros(prob.M)
    frame_obs = np.zeros(F, np.int64)
    margins = dict(cos=np.inf, window=np.inf, clip=np.inf)
    if clip_sigma > 0:
        n_r, mean_r, std_r = reference_of(ref)
        gate = clip_sigma * np.maximum(std_r, sigma_floor)
    for f in range(F):
        if use is not None and not use[f]:
            continue
        ok, I, cm, wm = observe(prob, frames[f], poses[f])
        margins["cos"] = min(margins["cos"], cm); margins["window"] = min(margins["window"], wm)
        keep = ok
        if clip_sigma > 0:
            judged = ok & (n_r > 0)
            d = np.abs(I - mean_r)
            if judged.any():
                margins["clip"] = min(margins["clip"], float(np.abs(d - gate)[judged].min()))
            keep = ok & ((n_r == 0) | (d <= gate))
            rej += ok & ~keep
        n += keep
        S += np.where(keep, I, 0.0)
        S2 += np.where(keep, I * I, 0.0)
        frame_obs[f] = int(keep.sum())
    return dict(n=n, S=S, S2=S2, rejected=rej, frame_obs=frame_obs, margins=margins)


def learn(prob, frames, poses, use=None, clip_sigma=1.5, sigma_floor=4.0):
    """the plain pass, then one clipped pass when clip_sigma > 0 -> (plain, final)"""
    plain = run_pass(prob, frames, poses, use)
    if not clip_sigma > 0:
        return plain, plain
    return plain, run_pass(prob, frames, poses, use, plain, clip_sigma, sigma_floor)


def template(result):
    """(mean (M,), NaN where n = 0)"""
    n, mean, _ = reference_of(result)
    return np.where(n > 0, mean, np.nan)


def margins_ok(m):
    return m["cos"] >= 1e-3 and m["window"] >= 1e-4 and m["clip"] >= 1e-6
