"""Calibrate the camera -- the CameraParams.npz every other tool takes as given -- from views of a planar target (include/agt_camcal.h).

:func:`calibrate_camera` has cv2.calibrateCamera's arguments and cost (1/2 sum |project - observed|^2 over the camera and one pose per
view); the minimiser is this project's Levenberg-Marquardt on the GPU (libagt_camcal.so), not OpenCV's CvLevMarq, so the two agree in
the minimum they reach and not in their iterates.  Without an intrinsic guess the start follows cv2's rule: principal point at the
image centre, no distortion, focal lengths by the closed form over per-view homographies (Zhang's two constraints per view on the image
of the absolute conic, as cvInitIntrinsicParams2D poses them; host numpy, normalised DLT).  The view poses come from ONE call of the
batched masked solvePnP of the per-frame library, which takes its planar-homography branch.

:func:`target_points_from_detections` turns a detection recording of a flat tag board into the per-view point lists,
:func:`target_points_from_chessboards` photographs of a printed chessboard (chessboard.find_chessboard finds the corners); corner
lists from elsewhere go into calibrate_camera directly.
"""
import numpy as np

from . import camcallib
from . import formats
from . import group_calib

# cv2's flag values
CALIB_USE_INTRINSIC_GUESS = 1
CALIB_FIX_ASPECT_RATIO = 2
CALIB_FIX_PRINCIPAL_POINT = 4
CALIB_ZERO_TANGENT_DIST = 8
CALIB_FIX_FOCAL_LENGTH = 16
CALIB_FIX_K1, CALIB_FIX_K2, CALIB_FIX_K3 = 32, 64, 128
CALIB_FIX_K4, CALIB_FIX_K5, CALIB_FIX_K6 = 2048, 4096, 8192
CALIB_RATIONAL_MODEL = 16384
CALIB_THIN_PRISM_MODEL = 32768
CALIB_FIX_S1_S2_S3_S4 = 65536
CALIB_USE_LU = 1 << 17
CALIB_TILTED_MODEL = 1 << 18
CALIB_FIX_TAUX_TAUY = 1 << 19
CALIB_USE_QR = 1 << 20
CALIB_FIX_TANGENT_DIST = 1 << 21

REFUSED_FLAGS = [(CALIB_TILTED_MODEL, "CALIB_TILTED_MODEL"), (CALIB_FIX_TAUX_TAUY, "CALIB_FIX_TAUX_TAUY"),
                 (CALIB_FIX_ASPECT_RATIO, "CALIB_FIX_ASPECT_RATIO"), (CALIB_USE_QR, "CALIB_USE_QR"), (CALIB_USE_LU, "CALIB_USE_LU")]
_KNOWN = (CALIB_USE_INTRINSIC_GUESS | CALIB_FIX_PRINCIPAL_POINT | CALIB_ZERO_TANGENT_DIST | CALIB_FIX_FOCAL_LENGTH | CALIB_FIX_K1 | CALIB_FIX_K2
          | CALIB_FIX_K3 | CALIB_FIX_K4 | CALIB_FIX_K5 | CALIB_FIX_K6 | CALIB_RATIONAL_MODEL | CALIB_THIN_PRISM_MODEL | CALIB_FIX_S1_S2_S3_S4
          | CALIB_FIX_TANGENT_DIST)

# entries of the camera vector (camcallib.CAMERA_NAMES)
FX, FY, CX, CY, K1, K2, P1, P2, K3, K4, K5, K6, S1, S2, S3, S4 = range(16)
MAX_POSE_POINTS = 256          # points per view the batched solvePnP of the start takes


def _bits(*idx):
    return sum(1 << i for i in idx)


def flags_to_mask(flags):
    """cv2.calibrateCamera flags -> (free mask over the camera vector, number of distortion coefficients returned: 5, 8 or 12).
    Raises cv_hip.error naming a flag this solver does not honour (tilted sensor, fixed aspect ratio, the solver-choice flags)."""
    flags = int(flags)
    for bit, name in REFUSED_FLAGS:
        if flags & bit:
            from . import cv_hip
            raise cv_hip.error("calibrateCamera: %s is not supported" % name)
    if flags & ~_KNOWN:
        from . import cv_hip
        raise cv_hip.error("calibrateCamera: unknown flag bits 0x%x" % (flags & ~_KNOWN))
    mask = _bits(FX, FY, CX, CY, K1, K2, P1, P2, K3)
    ndist = 5
    if flags & CALIB_RATIONAL_MODEL:
        mask |= _bits(K4, K5, K6); ndist = 8
    if flags & CALIB_THIN_PRISM_MODEL:
        mask |= _bits(S1, S2, S3, S4); ndist = 12
    fixed = 0
    if flags & CALIB_FIX_PRINCIPAL_POINT:
        fixed |= _bits(CX, CY)
    if flags & CALIB_FIX_FOCAL_LENGTH:
        fixed |= _bits(FX, FY)
    if flags & (CALIB_ZERO_TANGENT_DIST | CALIB_FIX_TANGENT_DIST):
        fixed |= _bits(P1, P2)
    for bit, i in ((CALIB_FIX_K1, K1), (CALIB_FIX_K2, K2), (CALIB_FIX_K3, K3), (CALIB_FIX_K4, K4), (CALIB_FIX_K5, K5), (CALIB_FIX_K6, K6)):
        if flags & bit:
            fixed |= 1 << i
    if flags & CALIB_FIX_S1_S2_S3_S4:
        fixed |= _bits(S1, S2, S3, S4)
    return mask & ~fixed, ndist


def camera_vector(camera_matrix, dist_coeffs=None):
    """(3, 3) matrix and 0, 4, 5, 8 or 12 coefficients -> c[16]; 14 (the tilted model) is CamCalError(ERR_CAMERA)"""
    K = np.asarray(camera_matrix, np.float64).reshape(3, 3)
    c = np.zeros(camcallib.NCAM)
    c[:4] = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    if dist_coeffs is not None:
        d = np.asarray(dist_coeffs, np.float64).reshape(-1)
        if d.size not in (0, 4, 5, 8, 12):
            raise camcallib.CamCalError(camcallib.ERR_CAMERA, "calibrate_camera (%d distortion coefficients)" % d.size)
        c[4:4 + d.size] = d
    return c


def camera_from_vector(c, ndist=12):
    """c[16] -> (mtx (3, 3), dist (1, ndist))"""
    return np.array([[c[0], 0.0, c[2]], [0.0, c[1], c[3]], [0.0, 0.0, 1.0]]), np.array(c[4:4 + ndist], np.float64).reshape(1, -1)


def homography_dlt(plane_xy, pixels):
    """The homography plane -> image of n >= 4 correspondences by the normalised DLT (both point sets moved to their centroid and
    scaled to a mean distance of sqrt 2; the null vector of the 2n x 9 system by numpy's SVD) -> H (3, 3), or None when a set
    collapses to a point"""
    M = np.asarray(plane_xy, np.float64).reshape(-1, 2); m = np.asarray(pixels, np.float64).reshape(-1, 2)

    def normalise(p):
        c = p.mean(axis=0)
        s = np.sqrt(((p - c) ** 2).sum(axis=1)).mean()
        if not s > 0.0:
            return None, None
        T = np.array([[np.sqrt(2.0) / s, 0.0, -c[0] * np.sqrt(2.0) / s], [0.0, np.sqrt(2.0) / s, -c[1] * np.sqrt(2.0) / s], [0.0, 0.0, 1.0]])
        return (p - c) * (np.sqrt(2.0) / s), T
    Mn, TM = normalise(M); mn, Tm = normalise(m)
    if Mn is None or mn is None:
        return None
    n = len(Mn)
    L = np.zeros((2 * n, 9))
    L[0::2, 0:2] = Mn; L[0::2, 2] = 1.0; L[0::2, 6:8] = -mn[:, 0:1] * Mn; L[0::2, 8] = -mn[:, 0]
    L[1::2, 3:5] = Mn; L[1::2, 5] = 1.0; L[1::2, 6:8] = -mn[:, 1:2] * Mn; L[1::2, 8] = -mn[:, 1]
    _, _, Vt = np.linalg.svd(L)
    H = np.linalg.inv(Tm) @ Vt[-1].reshape(3, 3) @ TM
    return H / H[2, 2] if H[2, 2] != 0.0 else H


def initial_focal_lengths(object_points, image_points, principal_point):
    """fx, fy from the views' homographies with the principal point known (the closed form cvInitIntrinsicParams2D uses).  With the
    principal point moved to the origin, H = [h1 h2 h3] ~ K [r1 r2 t] and r1 . r2 = 0, |r1| = |r2| give per view two equations that
    are linear in (1 / fx^2, 1 / fy^2); they are posed on the normalised columns h1, h2 and their normalised half sum and half
    difference, and solved over all views by least squares.  -> (fx, fy); CamCalError(ERR_DEGENERATE) when the estimate is not finite
    and positive (every view parallel to the sensor leaves the equations empty)."""
    cx, cy = principal_point
    A, b = [], []
    for X, m in zip(object_points, image_points):
        H = homography_dlt(np.asarray(X, np.float64).reshape(-1, 3)[:, :2], m)
        if H is None or not np.isfinite(H).all():
            continue
        H = H.copy()
        H[0] -= cx * H[2]; H[1] -= cy * H[2]
        h, v = H[:, 0], H[:, 1]
        d1, d2 = 0.5 * (h + v), 0.5 * (h - v)
        h, v, d1, d2 = (q / np.linalg.norm(q) for q in (h, v, d1, d2))
        A.append([h[0] * v[0], h[1] * v[1]]); b.append(-h[2] * v[2])
        A.append([d1[0] * d2[0], d1[1] * d2[1]]); b.append(-d1[2] * d2[2])
    bad = camcallib.CamCalError(camcallib.ERR_DEGENERATE, "calibrate_camera (no focal length from the views' homographies)")
    if len(A) < 2:
        raise bad
    A, b = np.asarray(A), np.asarray(b)
    sv = np.linalg.svd(A, compute_uv=False)
    if not np.isfinite(sv).all() or not sv[-1] > 1e-9 * sv[0]:
        raise bad
    f = np.linalg.lstsq(A, b, rcond=None)[0]
    if not (np.isfinite(f).all() and (f > 0.0).all()):
        raise bad
    fx, fy = 1.0 / np.sqrt(f)
    if not (np.isfinite(fx) and np.isfinite(fy)):
        raise bad
    return float(fx), float(fy)


def initial_view_poses(object_points, image_points, camera):
    """The pose of every view under camera c[16] in ONE call of the batched masked solvePnP (views padded to the longest) -> (V, 6)"""
    import torch
    from . import cv_hip
    cv_hip._require_gpu()
    V, n = len(object_points), max(len(o) for o in object_points)
    if n > MAX_POSE_POINTS:
        raise ValueError("calibrate_camera: a view has %d points; the start's solvePnP takes %d (thin the view)" % (n, MAX_POSE_POINTS))
    obj = np.zeros((V, n, 3)); img = np.zeros((V, n, 2)); mask = np.zeros((V, n), np.uint8)
    for v, (o, m) in enumerate(zip(object_points, image_points)):
        obj[v, :len(o)] = o; obj[v, len(o):] = o[0]
        img[v, :len(o)] = m; img[v, len(o):] = m[0]
        mask[v, :len(o)] = 1
    K, dist = camera_from_vector(camera)
    ctx = cv_hip._geom_context(n)
    with ctx.lock:
        ctx.use_current_stream()
        dev = torch.device("cuda", ctx.device)
        pose, info, _ = ctx.solve_pnp(torch.from_numpy(obj).to(dev), torch.from_numpy(img).to(dev), K, dist.reshape(-1) if np.any(dist) else None,
                                      mask=torch.from_numpy(mask).to(dev))
        pose = pose.cpu().numpy(); good = info.cpu().numpy()[:, 0] != 0
    if not good.all() or not np.isfinite(pose).all():
        raise camcallib.CamCalError(camcallib.ERR_DEGENERATE, "calibrate_camera (no pose for view %d)" % int(np.argmin(good)))
    return pose


def calibrate_camera(object_points, image_points, image_size, camera_matrix=None, dist_coeffs=None, flags=0, max_iters=100, ftol=None):
    """object_points / image_points: per view (n_v, 3) target coordinates and (n_v, 2) pixels; image_size (w, h); flags: cv2's CALIB_*.
    -> (rms, mtx (3, 3), dist (1, k), rvecs (V, 3), tvecs (V, 3), report dict).  rms is cv2's: sqrt(sum |r|^2 / points).
    Without CALIB_USE_INTRINSIC_GUESS the target must be planar (z = 0) and seen in at least three views; camera_matrix and
    dist_coeffs are then ignored (a coefficient fixed by a flag stays 0).  Raises camcallib.CamCalError on a refusal."""
    mask, nk = flags_to_mask(flags)
    obj = [np.ascontiguousarray(np.asarray(o, np.float64).reshape(-1, 3)) for o in object_points]
    img = [np.ascontiguousarray(np.asarray(m, np.float64).reshape(-1, 2)) for m in image_points]
    if len(obj) != len(img) or any(len(o) != len(m) for o, m in zip(obj, img)):
        raise ValueError("calibrate_camera: object and image points do not match")
    w, h = float(image_size[0]), float(image_size[1])
    guess = bool(int(flags) & CALIB_USE_INTRINSIC_GUESS)
    if guess:
        if camera_matrix is None:
            raise ValueError("calibrate_camera: CALIB_USE_INTRINSIC_GUESS needs camera_matrix")
        c0 = camera_vector(camera_matrix, dist_coeffs)
        if int(flags) & CALIB_ZERO_TANGENT_DIST:
            c0[[P1, P2]] = 0.0
    else:
        if any(np.any(o[:, 2] != 0.0) for o in obj):
            raise camcallib.CamCalError(camcallib.ERR_ARG, "calibrate_camera (a target that is not planar, z = 0, needs CALIB_USE_INTRINSIC_GUESS)")
        if len(obj) < 3:
            raise camcallib.CamCalError(camcallib.ERR_TOO_FEW, "calibrate_camera (fewer than 3 views and no intrinsic guess)")
    # the library's checks come first: a refusal costs no GPU work
    solver = camcallib.CamCal(obj, img, mask, nk)
    try:
        if not guess:
            c0 = np.zeros(camcallib.NCAM)
            c0[CX], c0[CY] = 0.5 * (w - 1.0), 0.5 * (h - 1.0)
            c0[FX], c0[FY] = initial_focal_lengths(obj, img, (c0[CX], c0[CY]))
        poses0 = initial_view_poses(obj, img, c0)
        c1, poses1, rep = solver.solve(c0, poses0, max_iters=int(max_iters), ftol=ftol)
        res, _ = solver.eval(c1, poses1)
    finally:
        solver.close()
    start = np.concatenate([[0], np.cumsum([len(o) for o in obj])])
    sq = (res * res).sum(axis=1)
    per_view = np.array([np.sqrt(sq[a:b].mean()) for a, b in zip(start[:-1], start[1:])])
    rms = float(np.sqrt(2.0 * rep.final_cost / len(sq)))
    mtx, dist = camera_from_vector(c1, nk)
    report = {
        "iterations": rep.iterations, "accepted": rep.accepted, "initial_cost": rep.initial_cost, "final_cost": rep.final_cost,
        "final_rms_px": rep.final_rms_px, "final_lambda": rep.final_lambda, "stop_reason": camcallib.STOP_NAMES.get(rep.stop_reason, "?"),
        "n_views": len(obj), "n_points": int(len(sq)), "free_mask": int(mask), "free": [n for i, n in enumerate(camcallib.CAMERA_NAMES) if mask >> i & 1],
        "rms": rms, "per_view_rms": per_view, "camera": c1, "initial_camera": c0, "initial_view_poses": poses0,
    }
    return rms, mtx, dist, poses1[:, :3].copy(), poses1[:, 3:].copy(), report


def target_points_from_detections(frames, board, decision_margin=formats.DECISION_MARGIN):
    """A detection recording (formats.load_detections) of a flat tag board -> (object_points, image_points, frame_index): per used
    frame the (4 m, 3) board coordinates (z = 0) and (4 m, 2) pixels of the corners of its m >= 1 accepted tags, and the frame's index in
    the recording.  board: an april_group dict ({"tags": {id: {"size", "extrinsics"}}} or formats.load_april_group's) whose tags lie in
    one plane; detections are filtered as group_calib.observation_table does (decision margin, tags of the board only, last record of
    a tag in a frame wins).  A board whose plane is not z = const is moved into it (a rigid motion of the target changes no camera)."""
    tags = board["tags"] if isinstance(board, dict) and "tags" in board else board
    tag_ids = sorted(int(t) for t in tags)
    sizes = []
    for t in tag_ids:
        v = tags[t] if t in tags else tags[str(t)]
        sizes.append(float(v["size"] if isinstance(v, dict) else v[0]))
    pts = group_calib.object_points(group_calib.group_to_poses(tags, tag_ids), sizes)
    if np.ptp(pts[:, 2]) == 0.0:
        pts = pts - [0.0, 0.0, pts[0, 2]]
    else:
        c = pts.mean(axis=0)
        _, s, Vt = np.linalg.svd(pts - c)
        if s[2] > 1e-6 * s[1]:
            raise ValueError("target_points_from_detections: the board's tags do not lie in one plane")
        if np.linalg.det(Vt) < 0:
            Vt = -Vt
        pts = (pts - c) @ Vt.T
        pts[:, 2] = 0.0
    pts = pts.reshape(-1, 4, 3)
    fr, tg, co = group_calib.observation_table(frames, tag_ids, decision_margin)
    obj, img, used = [], [], []
    for f in sorted(set(fr.tolist())):
        rows = np.nonzero(fr == f)[0]
        obj.append(pts[tg[rows]].reshape(-1, 3)); img.append(co[rows].reshape(-1, 2)); used.append(int(f))
    return obj, img, used


def chessboard_object_points(pattern_size, square_size):
    """(nx ny, 3): (i square, j square, 0) row by row, i = 0..nx-1 along a row -- the reference's objp (calibrate_camera.py:93-98)"""
    nx, ny = int(pattern_size[0]), int(pattern_size[1])
    if nx < 2 or ny < 2 or not float(square_size) > 0.0:
        raise ValueError("chessboard_object_points: a pattern of at least 2 x 2 inner corners and a square size > 0 are needed")
    i, j = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64))
    return np.stack([i.ravel() * float(square_size), j.ravel() * float(square_size), np.zeros(nx * ny)], axis=1)


def target_points_from_chessboards(images, pattern_size, square_size, find=None, **options):
    """Photographs of a chessboard -> (object_points, image_points, image_index), in the shapes target_points_from_detections returns:
    per image in which the whole board was found the (nx ny, 3) object points (i square, j square, 0) and the (nx ny, 2) corners, and
    the image's index.  images: host u8 frames, gray (H, W) or BGR (H, W, 3), of any sizes.  pattern_size: the INNER corners (nx, ny).
    find: gray (H, W) u8 -> (found, corners), cv_hip.findChessboardCorners' contract (that function when None; options go to it)."""
    pts = chessboard_object_points(pattern_size, square_size)
    if find is None:
        from . import cv_hip
        find = lambda gray: cv_hip.findChessboardCorners(gray, pattern_size, **options)
    obj, img, used = [], [], []
    for k, frame in enumerate(images):
        a = np.asarray(frame)
        if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
            raise ValueError("target_points_from_chessboards: image %d is not an 8-bit gray or BGR frame" % k)
        if a.ndim == 3:
            # cv2's BGR2GRAY weights in its 14-bit fixed point; host numpy: a calibration reads each photograph once
            a = ((a[..., 0].astype(np.int32) * 1868 + a[..., 1].astype(np.int32) * 9617 + a[..., 2].astype(np.int32) * 4899 + 8192) >> 14).astype(np.uint8)
        found, corners = find(np.ascontiguousarray(a))
        if found:
            obj.append(pts.copy()); img.append(np.asarray(corners, np.float64).reshape(-1, 2)); used.append(k)
    return obj, img, used


def format_report(report):
    rows = ["views used         : %d" % report["n_views"], "points             : %d" % report["n_points"],
            "estimated          : %s" % " ".join(report["free"]),
            "LM iterations      : %d (%d accepted), stopped: %s" % (report["iterations"], report["accepted"], report["stop_reason"]),
            "cost 1/2 sum r^2   : %.6g -> %.6g" % (report["initial_cost"], report["final_cost"]),
            "final RMS          : %.4f px" % report["rms"]]
    rows += ["RMS view %-4d      : %.4f px" % (i, e) for i, e in enumerate(report["per_view_rms"])]
    return "\n".join(rows)
