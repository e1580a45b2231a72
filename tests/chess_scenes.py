"""Rendered chessboards (TEST INFRASTRUCTURE): a board of (nx + 1) x (ny + 1) squares with a white margin one square wide on a gray
background, seen through tests/camera_calib_numpy.project's camera model -- every pixel sample is taken back through the lens by the
fixed-point inversion synthetic._undistort_norm uses and intersected with the board's plane -- 4 x 4 supersampled where a pixel's
neighbourhood meets an edge, 3 x 3 blurred, with optional seeded noise, u8.  Each frame comes with the true positions of its nx x ny
inner corners, row by row, nx along a row (camcal_scenes.grid's order).  The poses are camcal_scenes.view_poses'."""
import functools

import numpy as np
from scipy import ndimage
from scipy.spatial.transform import Rotation

import camcal_scenes as cs
import camera_calib_numpy as cn

BLACK, WHITE, GRAY = 30.0, 225.0, 128.0
PATTERN = (9, 6)
PITCH = 0.025
FILL = 0.55                 # of the image width, for the corner grid's extent: the whole board with its margin stays inside the frame
NOISE = 2.0                 # gray levels, sigma
SS = 4


def _undistort(xd, yd, k, tol=1e-10, iters=80):
    """the fixed-point inversion of the 5-coefficient lens, as synthetic._undistort_norm iterates it, stopped when it stands still"""
    k1, k2, p1, p2, k3 = k
    x, y = xd.copy(), yd.copy()
    with np.errstate(all="ignore"):
        for _ in range(iters):
            r2 = x * x + y * y
            icd = 1.0 / (1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 ** 3)
            dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
            dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
            xn, yn = (xd - dx) * icd, (yd - dy) * icd
            still = np.nanmax(np.maximum(np.abs(xn - x), np.abs(yn - y))) < tol
            x, y = xn, yn
            if still:
                break
    return x, y


def board_coordinates(cam, pose, px, py, pattern=PATTERN, pitch=PITCH):
    """pixel positions -> (a, b): board coordinates in squares, the squares being [k, k + 1) for k = 0..nx and 0..ny"""
    assert not np.any(cam[9:]), "the renderer inverts the 5-coefficient lens"
    x, y = _undistort((px - cam[2]) / cam[0], (py - cam[3]) / cam[1], cam[4:9])
    R = Rotation.from_rotvec(pose[:3]).as_matrix()
    t = pose[3:]
    n = R[:, 2]
    with np.errstate(all="ignore"):
        s = (n @ t) / (n[0] * x + n[1] * y + n[2])
        X = np.stack([s * x - t[0], s * y - t[1], s - t[2]], axis=-1) @ R           # R^T (s d - t)
    return X[..., 0] / pitch + (pattern[0] + 1) / 2.0, X[..., 1] / pitch + (pattern[1] + 1) / 2.0


def _cells(a, b, pattern):
    bad = ~(np.isfinite(a) & np.isfinite(b))
    ka = np.clip(np.floor(np.where(bad, -9.0, a)), -2, pattern[0] + 2).astype(int)
    kb = np.clip(np.floor(np.where(bad, -9.0, b)), -2, pattern[1] + 2).astype(int)
    return ka, kb


def _colour(ka, kb, pattern):
    board = (ka >= 0) & (ka <= pattern[0]) & (kb >= 0) & (kb <= pattern[1])
    margin = (ka >= -1) & (ka <= pattern[0] + 1) & (kb >= -1) & (kb <= pattern[1] + 1)
    return np.where(board, np.where((ka + kb) % 2 == 0, BLACK, WHITE), np.where(margin, WHITE, GRAY))


def truth(cam, pose, pattern=PATTERN, pitch=PITCH):
    return cn.project(cam, pose, cs.grid(pattern[0], pattern[1], pitch))


def render(cam, pose, size, pattern=PATTERN, pitch=PITCH, noise=0.0, seed=0, blur=True):
    """-> (frame u8 (H, W), corners (nx ny, 2))"""
    W, H = size
    e = np.linspace(-1.0, 1.0, 65)
    hx, hy = (pattern[0] + 3) / 2.0 * pitch, (pattern[1] + 3) / 2.0 * pitch
    outline = np.concatenate([np.stack([e * hx, np.full_like(e, s * hy)], 1) for s in (-1, 1)] + [np.stack([np.full_like(e, s * hx), e * hy], 1) for s in (-1, 1)])
    o = cn.project(cam, pose, np.concatenate([outline, np.zeros((len(outline), 1))], axis=1))
    x0, y0 = np.maximum(np.floor(o.min(axis=0)).astype(int) - 3, 0)
    x1, y1 = np.minimum(np.ceil(o.max(axis=0)).astype(int) + 3, [W - 1, H - 1])
    img = np.full((H, W), GRAY)
    if x1 >= x0 and y1 >= y0:
        px, py = np.meshgrid(np.arange(x0, x1 + 1, dtype=np.float64), np.arange(y0, y1 + 1, dtype=np.float64))
        ka, kb = _cells(*board_coordinates(cam, pose, px, py, pattern, pitch), pattern)
        box = _colour(ka, kb, pattern)
        label = ka * 64 + kb
        edge = ndimage.maximum_filter(label, 3, mode="nearest") != ndimage.minimum_filter(label, 3, mode="nearest")
        offs = (np.arange(SS) + 0.5) / SS - 0.5
        ex, ey = px[edge], py[edge]
        acc = np.zeros(len(ex))
        for oy in offs:
            for ox in offs:
                acc += _colour(*_cells(*board_coordinates(cam, pose, ex + ox, ey + oy, pattern, pitch), pattern), pattern)
        box[edge] = acc / (SS * SS)
        img[y0:y1 + 1, x0:x1 + 1] = box
    if blur:
        k = np.array([1.0, 2.0, 1.0]) / 4.0
        img = ndimage.convolve1d(ndimage.convolve1d(img, k, axis=0, mode="nearest"), k, axis=1, mode="nearest")
    if noise:
        img = img + noise * np.random.default_rng(seed + 4409).standard_normal(img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8), truth(cam, pose, pattern, pitch)


# ---- the scene classes of the tests: camera, frame size, seed of the poses, views
CLASSES = {"cam5": (cs.CAM5, cs.SIZE, 41, 6), "e2e": (cs.E2E_CAM, cs.E2E_SIZE, 43, 4)}


@functools.lru_cache(maxsize=None)
def poses(name, count=None):
    cam, size, seed, views = CLASSES[name]
    extent = (PATTERN[0] - 1) * PITCH
    return cs.view_poses(count or views, extent, cam, size, np.random.default_rng(seed), fill=FILL)


@functools.lru_cache(maxsize=None)
def view(name, k, noisy=False, count=None):
    """view k of a class -> (frame, true corners); read-only"""
    cam, size, seed, _ = CLASSES[name]
    frame, corners = render(cam, poses(name, count)[k], size, noise=NOISE if noisy else 0.0, seed=1000 * seed + k)
    frame.setflags(write=False); corners.setflags(write=False)
    return frame, corners


def class_views(name, noisy=False):
    return [view(name, k, noisy) for k in range(CLASSES[name][3])]


N_CAL, N_HELD = 12, 4


def calibration_views():
    """N_CAL + N_HELD views of the 640 x 480 camera, noisy"""
    return [view("cam5", k, True, N_CAL + N_HELD) for k in range(N_CAL + N_HELD)]


def half_outside():
    """the board of cam5's view 0 moved so that half of it lies outside the frame"""
    cam, size, seed, _ = CLASSES["cam5"]
    p = poses("cam5")[0].copy()
    p[3] += 0.8 * (PATTERN[0] - 1) * PITCH
    frame, corners = render(cam, p, size)
    outside = int((corners[:, 0] > size[0] - 1).sum())
    assert 14 <= outside <= 40, outside         # between a quarter and three quarters of the 54 corners
    return frame


def lattice(nx, ny, pitch=40.0, origin=(100.0, 80.0), roll_deg=0.0, shear=0.05):
    """bare points of an nx x ny grid, row by row with the row direction turned by roll_deg on the screen (x right, y down) about
    the grid's centre, slightly sheared and foreshortened so that it is no perfect square lattice -> (nx ny, 2) in the order the
    grid was laid out in (NOT necessarily the canonical one)"""
    i, j = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64))
    x = pitch * (i + shear * j) * (1.0 + 0.01 * i)
    y = pitch * 0.9 * j * (1.0 + 0.012 * j)
    p = np.stack([x.ravel(), y.ravel()], axis=1)
    c = p.mean(axis=0)
    t = np.deg2rad(roll_deg)
    Rm = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
    return (p - c) @ Rm.T + c + np.asarray(origin)


def canonical(points, a, b, nx, ny):
    """what the ordering rule asks of a grid laid out row by row with `a` points along each of its `b` rows, for the pattern (nx, ny):
    of its four turns in the plane those with nx along a row and a positive cross product of row and column direction, and among them
    the one whose first corner has the smallest x + y, ties to the smaller y"""
    A = np.asarray(points).reshape(b, a, 2)
    options = []
    for t in (A, A[::-1].transpose(1, 0, 2), A[::-1, ::-1], A[:, ::-1].transpose(1, 0, 2)):
        r, c = t[0, 1] - t[0, 0], t[1, 0] - t[0, 0]
        if t.shape[:2] == (ny, nx) and r[0] * c[1] - r[1] * c[0] > 0:
            options.append(t)
    best = min(options, key=lambda t: (t[0, 0, 0] + t[0, 0, 1], t[0, 0, 1]))
    return best.reshape(-1, 2)
