"""Calibrate an AprilGroup -- the april_group.json the tracker reads -- from a detection recording (include/agt_calib.h).

The reference needs the 6-DoF extrinsics of every tag on the tracked body and ships neither the file nor a way to make one.
:func:`calibrate_group` takes a recording of detections (formats.load_detections), the known edge length of every tag and the camera,
and bundle-adjusts the tag poses together with the per-frame body poses on the GPU (libagt_calib.so).  One tag, the anchor, is held
fixed: without a nominal group the body frame IS the anchor tag's frame.

Without a nominal group the start comes from a bootstrap over entry points the per-frame library already has: every (frame, tag)
four-point problem through the batched solvePnP in one call, tags placed breadth-first from the anchor over the co-visibility graph,
frame poses from the masked batched solve over the placed tags.  A planar four-point pose has two minima, so for every edge of the
graph the relative poses of several co-visible frames are candidates and the one with the smallest summed reprojection error of the
new tag over ALL frames that see both tags is kept (batched projectPoints).
"""
import collections

import numpy as np
from scipy.spatial.transform import Rotation

from . import caliblib
from . import formats

MAX_CANDIDATES = 8


def tag_corners(size):
    """(4, 3) corners of a tag in its own frame, the reference's template order (transform_helper.get_initial_pts)"""
    r = size / 2.0
    return np.array([[-r, -r, 0.0], [-r, r, 0.0], [r, r, 0.0], [r, -r, 0.0]])


def _mat(pose):
    return Rotation.from_rotvec(np.asarray(pose[:3], np.float64)).as_matrix(), np.asarray(pose[3:], np.float64)


def _pose(R, t):
    return np.concatenate([Rotation.from_matrix(R).as_rotvec(), t])


def compose(a, b):
    """pose of a o b: x -> R_a (R_b x + t_b) + t_a"""
    Ra, ta = _mat(a); Rb, tb = _mat(b)
    return _pose(Ra @ Rb, Ra @ tb + ta)


def invert(a):
    Ra, ta = _mat(a)
    return _pose(Ra.T, -Ra.T @ ta)


def observation_table(frames, tag_ids, decision_margin=formats.DECISION_MARGIN):
    """frames (formats.load_detections) -> (obs_frame (n,) i32, obs_tag (n,) i32: index into tag_ids, corners (n, 4, 2) f64): the
    detections that pass the decision margin and whose tag is in tag_ids; for a tag reported twice in a frame the last record wins"""
    row = {int(t): i for i, t in enumerate(tag_ids)}
    fr, tg, co = [], [], []
    for f, dets in enumerate(frames):
        last = collections.OrderedDict()
        for d in dets:
            if d.decision_margin < decision_margin or int(d.tag_id) not in row:
                continue
            last[row[int(d.tag_id)]] = np.asarray(d.corners, np.float64).reshape(4, 2)
        for t, c in last.items():
            fr.append(f); tg.append(t); co.append(c)
    return np.asarray(fr, np.int32), np.asarray(tg, np.int32), np.asarray(co, np.float64).reshape(-1, 4, 2)


def group_to_poses(group, tag_ids):
    """april_group dict ({"tags": {id: {"size", "extrinsics": [t, r]}}} or formats.load_april_group's {id: [size, tvec, rvec]})
    -> (T, 6) rvec | tvec in the order of tag_ids"""
    tags = group["tags"] if isinstance(group, dict) and "tags" in group else group
    out = np.zeros((len(tag_ids), 6))
    for i, t in enumerate(tag_ids):
        v = tags[t] if t in tags else tags[str(t)]
        if isinstance(v, dict):
            ext = np.asarray(v["extrinsics"], np.float64)
            out[i, :3], out[i, 3:] = ext[-3:], ext[:3]
        else:
            out[i, :3], out[i, 3:] = np.asarray(v[2], np.float64).ravel(), np.asarray(v[1], np.float64).ravel()
    return out


def poses_to_group(tag_poses, tag_ids, sizes):
    """-> the april_group.json dict; extrinsics [tx ty tz rx ry rz] rounded to float32, which is what the reference reads"""
    tags = {}
    for i, t in enumerate(tag_ids):
        ext = [float(np.float32(v)) for v in (*tag_poses[i, 3:], *tag_poses[i, :3])]
        tags[str(int(t))] = {"size": float(sizes[i]), "extrinsics": ext}
    return {"tags": tags}


def object_points(tag_poses, sizes):
    """(4T, 3) f64 body-frame corners of the tags under (T, 6) poses"""
    pts = []
    for p, s in zip(tag_poses, sizes):
        R, t = _mat(p)
        pts.append(tag_corners(s) @ R.T + t)
    return np.concatenate(pts)


def _gpu():
    import torch
    from . import cv_hip
    cv_hip._require_gpu()
    return torch, cv_hip


def solve_tag_views(obs_tag, corners, sizes, K, dist):
    """Every (frame, tag) four-point problem in ONE batched solve -> (poses (n, 6) tag -> camera, ok (n,) bool)"""
    torch, cv_hip = _gpu()
    n = len(obs_tag)
    obj = np.stack([tag_corners(sizes[t]) for t in obs_tag]) if n else np.zeros((0, 4, 3))
    ctx = cv_hip._geom_context(4)
    with ctx.lock:
        ctx.use_current_stream()
        dev = torch.device("cuda", ctx.device)
        pose, info, _ = ctx.solve_pnp(torch.from_numpy(np.ascontiguousarray(obj)).to(dev), torch.from_numpy(np.ascontiguousarray(corners)).to(dev),
                                      K, dist)
        return pose.cpu().numpy(), info.cpu().numpy()[:, 0] != 0


def reprojection_errors(points, poses, K, dist, observed):
    """Batched projectPoints: points (B, m, 3) under poses (B, 6) against observed (B, m, 2) -> (B,) summed squared pixel error"""
    torch, cv_hip = _gpu()
    ctx = cv_hip._geom_context(4)
    with ctx.lock:
        ctx.use_current_stream()
        dev = torch.device("cuda", ctx.device)
        points = np.ascontiguousarray(points, np.float64); poses = np.ascontiguousarray(poses, np.float64)
        img = []
        for i in range(0, len(poses), 32768):           # (the batch is the launch grid's second dimension: at most 65535)
            out, _ = ctx.project_points(torch.from_numpy(points[i:i + 32768]).to(dev), torch.from_numpy(poses[i:i + 32768]).to(dev), K, dist)
            img.append(out.cpu().numpy())
        d = np.concatenate(img) - observed
    e = (d * d).sum(axis=(1, 2))
    return np.where(np.isfinite(e), e, np.inf)


def choose_relative_pose(candidates, size, body_from_cam_views, corners, K, dist):
    """The candidate pose (tag -> body) of a new tag with the smallest summed reprojection error over all frames that see it together
    with the placed tag.  candidates (C, 6); body_from_cam_views (m, 6): camera <- body of those frames as the placed tag gives it;
    corners (m, 4, 2): the new tag's observed corners there.  -> (index, errors (C,))"""
    C_, m = len(candidates), len(body_from_cam_views)
    pts = np.stack([tag_corners(size) @ _mat(c)[0].T + _mat(c)[1] for c in candidates])            # (C, 4, 3) body frame
    errs = reprojection_errors(np.repeat(pts, m, axis=0), np.tile(body_from_cam_views, (C_, 1)), K, dist, np.tile(corners, (C_, 1, 1)))
    errs = errs.reshape(C_, m).sum(axis=1)
    return int(np.argmin(errs)), errs


def bootstrap(obs_frame, obs_tag, corners, sizes, anchor, n_frames, K, dist, anchor_pose=None, max_candidates=MAX_CANDIDATES,
              extra_candidates=None):
    """Initial tag poses (T, 6) without a nominal group; extra_candidates: {tag index: [poses]} added to that tag's candidates
    (tests inject a flipped four-point pose here).  -> (tag_poses, chosen {tag: (candidate index, errors)})"""
    T = len(sizes)
    views, ok = solve_tag_views(obs_tag, corners, sizes, K, dist)
    of = {(int(f), int(t)): i for i, (f, t) in enumerate(zip(obs_frame, obs_tag)) if ok[i]}
    frames_of = [[] for _ in range(T)]
    for (f, t) in sorted(of):
        frames_of[t].append(f)
    tag_poses = np.zeros((T, 6))
    if anchor_pose is not None:
        tag_poses[anchor] = anchor_pose
    placed = {anchor}
    chosen = {}
    queue = collections.deque([anchor])
    while queue:
        a = queue.popleft()
        fa = set(frames_of[a])
        for b in range(T):
            if b in placed:
                continue
            both = [f for f in frames_of[b] if f in fa]
            if not both:
                continue
            # camera <- body in the frames that see both, as tag a gives it; candidates: b's pose in the body from up to max_candidates of them
            cam_body = np.stack([compose(views[of[(f, a)]], invert(tag_poses[a])) for f in both])
            pick = both if len(both) <= max_candidates else [both[i] for i in np.linspace(0, len(both) - 1, max_candidates).round().astype(int)]
            cands = [compose(invert(cam_body[both.index(f)]), views[of[(f, b)]]) for f in pick]
            if extra_candidates and b in extra_candidates:
                cands = cands + [np.asarray(c, np.float64) for c in extra_candidates[b]]
            k, errs = choose_relative_pose(np.stack(cands), sizes[b], cam_body, np.stack([corners[of[(f, b)]] for f in both]), K, dist)
            tag_poses[b] = cands[k]
            chosen[b] = (k, errs)
            placed.add(b)
            queue.append(b)
    if len(placed) < T:
        raise caliblib.CalibError(caliblib.ERR_DISCONNECTED, "bootstrap")
    return tag_poses, chosen


def frame_poses_from_group(obs_frame, obs_tag, corners, tag_poses, sizes, n_frames, K, dist):
    """Body poses of all frames by the masked batched solve over the tags' corners -> (F, 6); zeros for a frame without observations"""
    torch, cv_hip = _gpu()
    T = len(sizes)
    obj = object_points(tag_poses, sizes)
    img = np.zeros((n_frames, 4 * T, 2)); mask = np.zeros((n_frames, 4 * T), np.uint8)
    for f, t, c in zip(obs_frame, obs_tag, corners):
        img[f, 4 * t:4 * t + 4] = c
        mask[f, 4 * t:4 * t + 4] = 1
    ctx = cv_hip._geom_context(4 * T)
    with ctx.lock:
        ctx.use_current_stream()
        dev = torch.device("cuda", ctx.device)
        pose, info, _ = ctx.solve_pnp(torch.from_numpy(obj).to(dev), torch.from_numpy(img).to(dev), K, dist, mask=torch.from_numpy(mask).to(dev))
        pose = pose.cpu().numpy(); good = info.cpu().numpy()[:, 0] != 0
    pose[~good] = 0.0
    return pose


def calibrate_group(frames, tag_sizes, cameraMatrix, distCoeffs, init_group=None, anchor=None, max_iters=50, ftol=None,
                    decision_margin=formats.DECISION_MARGIN, max_candidates=MAX_CANDIDATES):
    """frames: formats.load_detections(...); tag_sizes: {tag_id: edge length}; init_group: a nominal april_group dict (or None: bootstrap);
    anchor: the tag id held fixed (default: the tag seen in the most frames).
    -> (group_dict for formats.save_april_group, rvecs (F, 3), tvecs (F, 3), report dict).  Raises caliblib.CalibError on a refusal
    (disconnected co-visibility graph, fewer than two usable frames, unknown camera model)."""
    tag_ids = sorted(int(t) for t in tag_sizes)
    sizes = np.array([float(tag_sizes[t] if t in tag_sizes else tag_sizes[str(t)]) for t in tag_ids])
    K = np.ascontiguousarray(np.asarray(cameraMatrix, np.float64).reshape(3, 3))
    dist = None if distCoeffs is None else np.ascontiguousarray(np.asarray(distCoeffs, np.float64).reshape(-1))
    n_frames = len(frames)
    obs_frame, obs_tag, corners = observation_table(frames, tag_ids, decision_margin)
    seen = np.bincount(obs_tag, minlength=len(tag_ids))
    a = int(np.argmax(seen)) if anchor is None else tag_ids.index(int(anchor))
    # the library's checks come first: a refusal costs no GPU work
    solver = caliblib.GroupCalib(K, dist, sizes, a, n_frames, obs_frame, obs_tag, corners)
    try:
        if init_group is None:
            tag0, _ = bootstrap(obs_frame, obs_tag, corners, sizes, a, n_frames, K, dist, max_candidates=max_candidates)
        else:
            tag0 = group_to_poses(init_group, tag_ids)
        frame0 = frame_poses_from_group(obs_frame, obs_tag, corners, tag0, sizes, n_frames, K, dist)
        tag1, frame1, rep = solver.solve(tag0, frame0, max_iters=int(max_iters), ftol=ftol)
    finally:
        solver.close()
    report = {
        "iterations": rep.iterations, "accepted": rep.accepted, "initial_cost": rep.initial_cost, "final_cost": rep.final_cost,
        "final_rms_px": rep.final_rms_px, "final_lambda": rep.final_lambda, "stop_reason": caliblib.STOP_NAMES.get(rep.stop_reason, "?"),
        "n_observations": int(len(obs_tag)), "n_frames_used": int(len(np.unique(obs_frame))), "anchor": tag_ids[a], "tag_ids": tag_ids,
        "frames_per_tag": {tag_ids[i]: int(seen[i]) for i in range(len(tag_ids))},
        "tag_poses": tag1, "initial_tag_poses": tag0, "initial_frame_poses": frame0,
        "initial_group": poses_to_group(tag0, tag_ids, sizes),
    }
    return poses_to_group(tag1, tag_ids, sizes), frame1[:, :3].copy(), frame1[:, 3:].copy(), report


def format_report(report):
    rows = ["frames used        : %d" % report["n_frames_used"], "observations       : %d" % report["n_observations"],
            "anchor tag         : %s (its frame is the body frame unless a nominal group was given)" % report["anchor"],
            "LM iterations      : %d (%d accepted), stopped: %s" % (report["iterations"], report["accepted"], report["stop_reason"]),
            "cost 1/2 sum r^2   : %.6g -> %.6g" % (report["initial_cost"], report["final_cost"]),
            "final RMS          : %.4f px" % report["final_rms_px"], "final lambda       : %.3g" % report["final_lambda"],
            "frames per tag     : %s" % ", ".join("%s: %d" % kv for kv in sorted(report["frames_per_tag"].items()))]
    return "\n".join(rows)
