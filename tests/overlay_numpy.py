"""The drawing rule of include/agt_draw.h stated a second time, in numpy: per pixel, one primitive after the other over the whole frame,
int64 for everything that fits and Python integers for the squared cross product wherever int64 could not hold four times it.  It
shares no code with the binding and knows nothing of tiles, chunks or bounding boxes."""
import functools
import math

import numpy as np

NONE, DISC, SEGMENT = 0, 1, 2
MAX_COORD, MAX_SIZE = 32767, 64
PRIM_DTYPE = np.dtype([("kind", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("size", "<i4"), ("color", "u1", (4,)),
                       ("reserved", "<i4")])


def prim(kind, x0, y0, x1, y1, size, color):
    p = np.zeros((), PRIM_DTYPE)
    p["kind"], p["x0"], p["y0"], p["x1"], p["y1"], p["size"] = kind, x0, y0, x1, y1, size
    p["color"][:3] = color
    return p


def disc(x, y, r, color):
    return prim(DISC, x, y, x, y, r, color)


def segment(x0, y0, x1, y1, t, color):
    return prim(SEGMENT, x0, y0, x1, y1, t, color)


def prim_list(prims):
    return np.array(prims, PRIM_DTYPE) if len(prims) else np.zeros(0, PRIM_DTYPE)


def paints(p):
    return (int(p["kind"]) in (DISC, SEGMENT) and all(abs(int(p[k])) <= MAX_COORD for k in ("x0", "y0", "x1", "y1"))
            and 0 <= int(p["size"]) <= MAX_SIZE)


@functools.lru_cache(maxsize=4)
def _grid(width, height):
    py, px = np.mgrid[0:height, 0:width].astype(np.int64)
    return py, px


def coverage(p, width, height):
    """bool [height, width]: the pixels primitive p paints"""
    if not paints(p):
        return np.zeros((height, width), bool)
    py, px = _grid(width, height)
    ax, ay, bx, by, size = (int(p[k]) for k in ("x0", "y0", "x1", "y1", "size"))
    if int(p["kind"]) == DISC:
        return (px - ax) ** 2 + (py - ay) ** 2 <= size * size + size
    dx, dy = bx - ax, by - ay
    L2, T2 = dx * dx + dy * dy, size * size
    t = (px - ax) * dx + (py - ay) * dy
    head = 4 * ((px - ax) ** 2 + (py - ay) ** 2) <= T2
    tail = 4 * ((px - bx) ** 2 + (py - by) ** 2) <= T2
    cross = dx * (py - ay) - dy * (px - ax)                     # below 2^34: int64 holds it, not its square
    mid = (t > 0) & (t < L2)
    small = np.abs(cross) < (1 << 30)                           # 4 cross^2 < 2^62: int64 holds it; the others go through Python integers
    body = np.zeros((height, width), bool)
    body[small] = 4 * cross[small] ** 2 <= T2 * L2
    big = mid & ~small
    body[big] = [4 * int(c) * int(c) <= T2 * L2 for c in cross[big]]
    return np.where(t <= 0, head, np.where(t >= L2, tail, body))


def raster(frame, prims, clear=False):
    """frame u8 [H, W] or [H, W, 3], painted in place with prims (PRIM_DTYPE [P]) in list order -> frame"""
    h, w = frame.shape[:2]
    covered = np.zeros((h, w), bool)
    for p in prims:
        m = coverage(p, w, h)
        covered |= m
        frame[m] = p["color"][0] if frame.ndim == 2 else p["color"][:3]
    if clear:
        frame[~covered] = 0
    return frame


def pose_lists(points, width, height, gate=None, radius=5, thickness=5, dot_color=(0, 0, 255), line_color=(255, 255, 255)):
    """points [B, n, 2] f32 or f64, gate [B] f64 or None -> (dots, outline), PRIM_DTYPE [B, n] each"""
    pts = np.asarray(points).astype(np.float64)
    B, n = pts.shape[:2]
    dots, outline = np.zeros((B, n), PRIM_DTYPE), np.zeros((B, n), PRIM_DTYPE)
    for b in range(B):
        if gate is not None and not float(gate[b]) == 1.0:
            continue
        for i in range(n):
            x, y = float(pts[b, i, 0]), float(pts[b, i, 1])
            if math.isfinite(x) and math.isfinite(y):
                rx, ry = float(np.round(x)), float(np.round(y))
                if 0 <= rx < width and 0 <= ry < height:
                    dots[b, i] = disc(int(rx), int(ry), radius, dot_color)
        for g in range(0, n, 4):
            quad = pts[b, g:g + 4]
            if not np.isfinite(quad).all():
                continue
            q = [(int(u), int(v)) for u, v in quad]                 # int(): toward zero
            if any(u < 0 or u >= width or v < 0 or v >= height for u, v in q):
                continue
            for j in range(4):
                outline[b, g + j] = segment(q[j][0], q[j][1], q[(j + 1) % 4][0], q[(j + 1) % 4][1], thickness, line_color)
    return dots, outline


def draw_pose(frame, draw_frame, points, drawn=True, radius=5, thickness=5):
    """one entry of overlay.draw_pose on host arrays, in place: points [n, 2]"""
    h, w = frame.shape[:2]
    dots, outline = pose_lists(np.asarray(points)[None], w, h, None if drawn else np.zeros(1), radius, thickness)
    raster(frame, dots[0])
    raster(draw_frame, outline[0], clear=True)
    return frame, draw_frame
