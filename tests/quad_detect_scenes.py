"""Inputs of the quad finder's tests (CPU and GPU): patterns that break labelling kernels, single rendered quads, and the numpy chain
find -> refine on the tag scenes of tests/tag_decode_scenes.py (computed once per process and shared)."""
import functools

import numpy as np

import quad_detect_numpy as qd
import quad_refine_numpy as qn
import tag_decode_scenes as ts

TILE_W, TILE_H = 64, 16                      # the labelling workgroup's tile (csrc/agt_quadfind.hip)
# the sizes of the issue, then below / at / one above the tile in each direction
LABEL_SIZES = [(8, 8), (61, 45), (64, 48), (130, 70),
               (TILE_W - 1, TILE_H - 1), (TILE_W, TILE_H), (TILE_W + 1, TILE_H + 1), (TILE_W + 1, TILE_H - 1), (TILE_W - 1, TILE_H + 1)]
SCENE_FRAMES = [("small", 0), ("small", 1), ("small", 2), ("small", 3), ("c2", 0), ("c2", 1), ("dense", 0), ("dense", 1)]
RAW_PX, REFINED_PX, MAX_CANDIDATES = 3.0, 0.35, 512


def spiral(w, h):
    """a one-pixel line that winds inwards from (0, 0) with one clear pixel between its turns: one long component"""
    m = np.zeros((h, w), bool)
    x, y, dx, dy = 0, 0, 1, 0
    m[0, 0] = True

    def free(x, y, dx, dy):
        nx, ny, fx, fy = x + dx, y + dy, x + 2 * dx, y + 2 * dy
        if not (0 <= nx < w and 0 <= ny < h) or m[ny, nx]:
            return False
        return not (0 <= fx < w and 0 <= fy < h) or not m[fy, fx]

    for _ in range(w * h):
        if not free(x, y, dx, dy):
            dx, dy = -dy, dx                        # turn right (y runs down)
            if not free(x, y, dx, dy):
                break
        x, y = x + dx, y + dy
        m[y, x] = True
    return m


def comb(w, h):
    """teeth on every other column that meet only in the last row: the smallest index is far from the join"""
    m = np.zeros((h, w), bool)
    m[:, ::2] = True
    m[h - 1, :] = True
    return m


def u_shape(w, h):
    """two bars joined at the far end (the last column and row that lie in a full 4 x 4 tile: pixels beyond feed no tile)"""
    m = np.zeros((h, w), bool)
    x1, y1 = 4 * (w // 4) - 1, 4 * (h // 4) - 1
    m[:y1 + 1, 0] = m[:y1 + 1, x1] = True
    m[y1, :x1 + 1] = True
    return m


def serpentine(w, h):
    """every other row, joined at alternating ends: one component that crosses every vertical tile border on every other row"""
    m = np.zeros((h, w), bool)
    m[::2, :] = True
    for i, y in enumerate(range(1, h, 2)):
        if y + 1 < h:
            m[y, w - 1 if i % 2 == 0 else 0] = True
    return m


def diagonal_blobs(w, h):
    """two 3 x 3 blobs that touch only by a corner (at a tile corner where the frame has one): two components"""
    m = np.zeros((h, w), bool)
    cx = TILE_W if w > TILE_W + 3 else w // 2
    cy = TILE_H if h > TILE_H + 3 else h // 2
    m[cy - 3:cy, cx - 3:cx] = True
    m[cy:cy + 3, cx:cx + 3] = True
    return m


def checkerboard(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return (xx + yy) % 2 == 0


def uniform(w, h):
    return np.zeros((h, w), bool)


PATTERNS = [spiral, comb, u_shape, serpentine, diagonal_blobs, checkerboard, uniform]


def draw(mask):
    """0 where the pattern is, 255 elsewhere: with a clear pixel within every 4 x 4 tile's neighbourhood the dark mask is the pattern"""
    return np.where(mask, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def pattern_frames(w, h):
    """(frames u8 [P, h, w], masks bool [P, h, w], labels i32 [P, h, w] by the numpy statement)"""
    masks = np.stack([p(w, h) for p in PATTERNS])
    frames = np.stack([draw(m) for m in masks])
    labels = np.stack([qd.labels(f) for f in frames])
    for a in (masks, frames, labels):
        a.setflags(write=False)
    return frames, masks, labels


def scipy_labels(mask):
    """scipy.ndimage.label with 4-connectivity, relabelled to each component's smallest linear index; -1 elsewhere"""
    from scipy import ndimage
    lab, n = ndimage.label(mask, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    if n == 0:
        return np.full(mask.shape, -1, np.int32)
    index = np.arange(mask.size).reshape(mask.shape)
    smallest = np.asarray(ndimage.minimum(index, lab, np.arange(1, n + 1))).astype(np.int64)
    return np.where(lab > 0, np.concatenate([[-1], smallest])[lab], -1).astype(np.int32)


# ---- single rendered quads

def render_quad(w, h, quad, ss=4):
    """a black (30) convex quad on white (225), ss x ss supersampled"""
    q = np.asarray(quad, np.float64)
    sgn = np.sign(sum(q[e][0] * q[(e + 1) % 4][1] - q[(e + 1) % 4][0] * q[e][1] for e in range(4)))
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    cover = np.zeros((h, w))
    for oy in (np.arange(ss) + 0.5) / ss - 0.5:
        for ox in (np.arange(ss) + 0.5) / ss - 0.5:
            inside = np.ones((h, w), bool)
            for e in range(4):
                a, b = q[e], q[(e + 1) % 4]
                inside &= sgn * ((b[0] - a[0]) * (ys + oy - a[1]) - (b[1] - a[1]) * (xs + ox - a[0])) >= 0
            cover += inside
    return np.clip(np.rint(225 - 195 * cover / (ss * ss)), 0, 255).astype(np.uint8)


def square(half, turn_deg, centre):
    c, s = np.cos(np.deg2rad(turn_deg)), np.sin(np.deg2rad(turn_deg))
    base = np.array([[-1.0, -1.0], [1.0, -1.0], [1.0, 1.0], [-1.0, 1.0]]) * half          # clockwise on the screen
    return base @ np.array([[c, s], [-s, c]]) + np.asarray(centre, np.float64)


# (width, height, half-side, turn): the table of the issue
SINGLE_QUADS = [(64, 48, 12, 0.0), (64, 48, 12, 25.0), (70, 50, 14, 40.0), (200, 160, 30, 25.0), (400, 400, 150, 20.0)]


@functools.lru_cache(maxsize=None)
def single_quad(i):
    w, h, half, turn = SINGLE_QUADS[i]
    truth = square(half, turn, ((w - 1) / 2.0, (h - 1) / 2.0))
    return render_quad(w, h, truth), truth


@functools.lru_cache(maxsize=None)
def border_quads():
    """a 30-px half-side square turned by 25 degrees in a 200 x 160 frame, its extreme vertex 1 px outside each frame border
    (`touching`: dark pixels in the border row or column) and 1.5 px inside it (`inside`) -> list of (kind, frame, truth)"""
    w, h = 200, 160
    base = square(30, 25.0, (0.0, 0.0))
    ext = np.abs(base).max()
    out = []
    for poke, kind in ((1.0, "touching"), (-1.5, "inside")):
        for centre in ((ext - poke, 80.0), (w - 1 - ext + poke, 80.0), (100.0, ext - poke), (100.0, h - 1 - ext + poke)):
            truth = base + centre
            out.append((kind, render_quad(w, h, truth), truth))
    return out


def match_error(quad, truth):
    """the largest coordinate difference |dx|, |dy| between the quad and the true corners under the best rotation and orientation of
    the quad (the measure of the issue's tables: 1.83 / 2.68 / 2.17 px on small / c2 / dense) -> (error, the quad so arranged)"""
    best = (np.inf, None)
    for q in (np.asarray(quad, np.float64), np.asarray(quad, np.float64)[::-1]):
        for r in range(4):
            a = np.roll(q, r, axis=0)
            e = np.abs(a - truth).max()
            if e < best[0]:
                best = (e, a)
    return best


@functools.lru_cache(maxsize=None)
def numpy_chain(name, k):
    """the numpy statement's find on frame k of a scene, then quad_refine_numpy.refine_quad (defaults) on the candidate nearest each
    front tag -> dict(counts, quads, records, front, raw (per front tag: largest coordinate error of the nearest candidate),
    raw_l2, candidate (its slot), status, refined (per front tag: largest corner distance after refinement))"""
    seq = ts.sequence(name)
    img = seq.frame(k)
    quads, rec, counts = qd.detect(img)
    n = min(int(counts[2]), len(quads))
    truth = ts.quads(seq, k).astype(np.float64)
    front = ts.front_tags(seq, k)
    raw, raw_l2, cand, status, refined = [], [], [], [], []
    for t in front:
        errs = [match_error(quads[c], truth[t]) for c in range(n)]
        c = int(np.argmin([e[0] for e in errs]))
        raw.append(errs[c][0]); cand.append(c)
        raw_l2.append(np.linalg.norm(errs[c][1] - truth[t], axis=1).max())
        r = qn.refine_quad(img, quads[c])
        status.append(r["status"])
        refined.append(match_error(r["quad64"], truth[t])[1])
        refined[-1] = np.linalg.norm(refined[-1] - truth[t], axis=1).max()
    return dict(counts=counts, quads=quads, records=rec, front=front, raw=np.array(raw), raw_l2=np.array(raw_l2), candidate=np.array(cand),
                status=np.array(status), refined=np.array(refined))
