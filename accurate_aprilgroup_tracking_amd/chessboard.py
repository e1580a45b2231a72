"""Finding the inner corners of a chessboard (include/agt_chess.h -> libagt_chess.so, and the grid assembly on the host).

The method is this project's own -- a ring corner response, its local maxima, the saddle-point iteration behind cv2.cornerSubPix on
every maximum (all three on the device, integer or FP64 in a fixed order, so two runs give the same bits) and a grid grown along
nearest neighbours on the host.  It is not cv2's adaptive-threshold, erode and link-quads method; only the contract of
:func:`find_chessboard` and cv_hip.findChessboardCorners is cv2's: pattern size (nx, ny) in, found and nx ny corners out, row by row.
The sub-pixel step is for the X-corners of a chessboard only: a tag's L-corner has no saddle point (README.md), so nothing here is
offered to the tracker.
"""
import collections

import numpy as np

from . import _sidelib
from . import chesslib as Q

Corners = collections.namedtuple("Corners", "candidates counts records")
Corners.__doc__ = """ChessboardFinder.corners' result, all cuda tensors: candidates i32 [B, max_candidates, 3] (x, y, response, in
raster order), counts i32 [B, 4] (candidates before the cap, candidates written, the frame's largest response, flag bits), records u8
[B, max_candidates, 48] (records_numpy gives the fields: x, y, det, shift, xf, yf, verdict).  Entries behind counts[b, 1] are zero."""


class ChessboardFinder:
    """The workspace of the corner finder for frames of up to width x height in batches of up to max_batch; max_candidates: the
    candidates written per frame.  Calls on one ChessboardFinder share the workspace: issue them on one stream."""

    def __init__(self, width, height, max_batch=1, max_candidates=1024):
        self.width, self.height, self.max_batch, self.max_candidates = int(width), int(height), int(max_batch), int(max_candidates)
        for name, v, lo, hi in (("width", self.width, Q.MIN_SIZE, Q.MAX_SIZE), ("height", self.height, Q.MIN_SIZE, Q.MAX_SIZE),
                                ("max_batch", self.max_batch, 1, Q.MAX_BATCH), ("max_candidates", self.max_candidates, 1, Q.MAX_CANDIDATES)):
            if not lo <= v <= hi:
                raise Q.ChessError(Q.ERR_ARG, "ChessboardFinder(%s=%d), limits %d..%d" % (name, v, lo, hi))
        self._finder = _sidelib.PerDevice(Q.Finder, self.width, self.height, self.max_batch, self.max_candidates)

    def _call(self, frames):
        import torch
        from .cv_hip import _require_gpu
        _sidelib.check_frames(frames, Q.MIN_SIZE, self.width, self.height, self.max_batch, Q.ChessError, "ChessboardFinder")
        _require_gpu()
        dev = frames.device
        return torch, dev, self._finder(dev.index), _sidelib.frame_args(frames)

    def response(self, frames):
        """-> cuda i32 [B, H, W]: the corner response of every pixel (0 closer than 5 to a border).  Enqueues only."""
        torch, dev, fd, args = self._call(frames)
        out = torch.empty(tuple(frames.shape), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            fd.response(*args, out.data_ptr())
        return out

    def _outputs(self, torch, dev, B, records=True):
        c = torch.empty((B, self.max_candidates, 3), dtype=torch.int32, device=dev)
        n = torch.empty((B, 4), dtype=torch.int32, device=dev)
        r = torch.empty((B, self.max_candidates, Q.RECORD_DTYPE.itemsize), dtype=torch.uint8, device=dev) if records else None
        return c, n, r

    def candidates(self, frames, **options):
        """stages 1 and 2 -> (candidates, counts) as in Corners.  Enqueues only."""
        opts = Q.options(**options)
        torch, dev, fd, args = self._call(frames)
        c, n, _ = self._outputs(torch, dev, args[-1], records=False)
        with torch.cuda.device(dev):
            fd.candidates(*args, opts, c.data_ptr(), n.data_ptr())
        return c, n

    def refine(self, frames, candidates, counts, **options):
        """stage 3 on given seeds (cuda i32 [B, max_candidates, 3] and [B, 4], contiguous) -> records.  Enqueues only."""
        opts = Q.options(**options)
        torch, dev, fd, args = self._call(frames)
        B = args[-1]
        for t, shape in ((candidates, (B, self.max_candidates, 3)), (counts, (B, 4))):
            if not (isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.device == dev and tuple(t.shape) == shape and t.is_contiguous()):
                raise ValueError("seeds must be contiguous cuda i32 %s on the frames' device" % (shape,))
        r = torch.empty((B, self.max_candidates, Q.RECORD_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            fd.refine(*args, opts, candidates.data_ptr(), counts.data_ptr(), r.data_ptr())
        return r

    def corners(self, frames, **options):
        """frames: cuda u8 [B, H, W] (unit pixel stride; any row and frame stride).  options: min_response (200), rel_pct (10), nms (3),
        half (5), iters (10), max_shift (3.0), min_det (1.0).  Stages 1 to 3; enqueues on the current stream and returns a Corners
        without synchronising."""
        opts = Q.options(**options)
        torch, dev, fd, args = self._call(frames)
        out = Corners(*self._outputs(torch, dev, args[-1]))
        with torch.cuda.device(dev):
            fd.corners(*args, opts, out.candidates.data_ptr(), out.counts.data_ptr(), out.records.data_ptr())
        return out


def records_numpy(records):
    """records tensor (or its numpy copy) -> structured array [B, max_candidates] with the fields of agt_chess_record (synchronises)"""
    return _sidelib.records_numpy(records, Q.RECORD_DTYPE)


# ---- stage 4: the grid, on the host

GROW_TOL = 0.3          # a neighbour is taken within this fraction of the local step of where it is predicted
MID_TOL = 0.2           # an inner point lies within this fraction of the local step of the midpoint of its opposite neighbours
_STEPS = ((1, 0), (-1, 0), (0, 1), (0, -1))


def _bases(P, seed):
    """the pairs of steps (u, v) a lattice through point `seed` may start with: two of its six nearest neighbours (those that lie
    behind another point left out), the nearer first, between 53 and 127 degrees apart and the farther at most 2.5 times as far, v
    turned so that u x v > 0"""
    d = np.hypot(*(P - P[seed]).T)
    near = [int(k) for k in np.argsort(d, kind="stable")[1:7]]
    # a step that jumps over a point (one lies within a quarter of it of its middle) is two steps of the lattice, not one
    near = [k for k in near if d[k] > 0 and not np.any(np.hypot(*(P - 0.5 * (P[seed] + P[k])).T) < 0.25 * d[k])]
    for n, a in enumerate(near):
        u = P[a] - P[seed]
        lu = np.hypot(*u)
        for b in near[n + 1:]:
            v = P[b] - P[seed]
            lv = np.hypot(*v)
            if lu > 0 and abs(u @ v) < 0.6 * lu * lv and lv <= 2.5 * lu:
                yield u, (v if u[0] * v[1] - u[1] * v[0] > 0 else -v)


def _grow(P, seed, u, v, reach):
    """The lattice grown from point `seed` with the steps u and v: {(i, j): point index}.  A cell's neighbour is predicted from the
    step that led to the cell (or the one across it) and is the nearest point, taken when it is unused and lies within GROW_TOL of
    the step; `reach` bounds |i| and |j|, so the loop ends."""
    cells, used = {(0, 0): seed}, {seed}
    step = {(0, 0): {(1, 0): u, (-1, 0): -u, (0, 1): v, (0, -1): -v}}
    queue = collections.deque([(0, 0)])
    while queue:                                    # every cell enters once and the cells are bounded by reach
        c = queue.popleft()
        for s in _STEPS:
            n = (c[0] + s[0], c[1] + s[1])
            if n in cells or max(abs(n[0]), abs(n[1])) > reach:
                continue
            back = (c[0] - s[0], c[1] - s[1])
            e = P[cells[c]] - P[cells[back]] if back in cells else step[c][s]
            at = P[cells[c]] + e
            dist = np.hypot(*(P - at).T)
            k = int(np.argmin(dist))
            if k in used or dist[k] > GROW_TOL * np.hypot(*e):
                continue
            cells[n] = k; used.add(k)
            e = P[k] - P[cells[c]]
            mine = dict(step[c])                    # the cell inherits its parent's steps, the one just walked measured anew
            mine[s] = e; mine[(-s[0], -s[1])] = -e
            step[n] = mine
            queue.append(n)
    return cells


def _blocks(cells, w, h):
    """the places (i0, j0) of a lattice where a block of w x h cells is complete and stands alone: none of the four lines next to
    it is complete as well (a larger grid is not this pattern), while stray cells next to it -- false points that fell on a lattice
    place -- do not matter"""
    i_lo, i_hi = min(c[0] for c in cells), max(c[0] for c in cells)
    j_lo, j_hi = min(c[1] for c in cells), max(c[1] for c in cells)
    occ = np.zeros((i_hi - i_lo + 3, j_hi - j_lo + 3), bool)          # an empty line all round
    for i, j in cells:
        occ[i - i_lo + 1, j - j_lo + 1] = True
    for i in range(1, occ.shape[0] - w):
        for j in range(1, occ.shape[1] - h):
            if occ[i:i + w, j:j + h].all() and not (occ[i - 1, j:j + h].all() or occ[i + w, j:j + h].all() or
                                                    occ[i:i + w, j - 1].all() or occ[i:i + w, j + h].all()):
                yield i + i_lo - 1, j + j_lo - 1


def _irregularity(G):
    """the largest parallelogram defect of a unit cell of G, relative to the cell's mean side"""
    d = np.hypot(*(G[1:, 1:] - G[1:, :-1] - G[:-1, 1:] + G[:-1, :-1]).transpose(2, 0, 1))
    side = 0.25 * (np.hypot(*(G[1:, 1:] - G[1:, :-1]).transpose(2, 0, 1)) + np.hypot(*(G[:-1, 1:] - G[:-1, :-1]).transpose(2, 0, 1)) +
                   np.hypot(*(G[1:, 1:] - G[:-1, 1:]).transpose(2, 0, 1)) + np.hypot(*(G[1:, :-1] - G[:-1, :-1]).transpose(2, 0, 1)))
    return float((d / side).max())


def _consistent(G):
    """local consistency of a grid G [rows, cols, 2]: every point with two opposite neighbours lies near their midpoint"""
    for A in (G, G.transpose(1, 0, 2)):
        if A.shape[1] >= 3:
            mid = 0.5 * (A[:, :-2] + A[:, 2:])
            half = 0.5 * np.hypot(*(A[:, 2:] - A[:, :-2]).transpose(2, 0, 1))
            off = np.hypot(*(A[:, 1:-1] - mid).transpose(2, 0, 1))
            if np.any(off > MID_TOL * half):
                return False
    return True


def assemble(points, ok, pattern_size):
    """points (N, 2), ok (N,) truth values (None = all good), pattern_size (nx, ny) -> (found, corners (nx ny, 2) float64).
    The corners run row by row with nx points along a row; the order is never mirrored (the image-plane cross product of the row and
    column directions is positive); among the admissible rotations (two when nx != ny, four when nx == ny) it is the one whose first
    corner has the smallest x + y, a tie going to the smaller y.  found is False (and corners all zero) when no grid of exactly that
    size can be completed: a missing corner means not found, extra points that belong to no grid do not break a complete board.
    The grid is verified point by point against its neighbours, never by one homography: a distorting lens bends the rows."""
    nx, ny = int(pattern_size[0]), int(pattern_size[1])
    if nx < 2 or ny < 2:
        raise ValueError("assemble: pattern_size must be at least 2 x 2")
    P = np.asarray(points, np.float64).reshape(-1, 2)
    if ok is not None:
        P = P[np.asarray(ok).reshape(-1).astype(bool)]
    none = (False, np.zeros((nx * ny, 2)))
    if len(P) < nx * ny or not np.isfinite(P).all():
        return none
    # nine points do not fall into a consistent lattice by chance: the first grid found is the board.  Four or six may, among false
    # points: for such a pattern every seed is tried and the most regular grid is the board
    exhaustive = nx * ny < 9
    best = None
    for seed in range(len(P)):
        for u, v in _bases(P, seed):
            cells = _grow(P, seed, u, v, max(nx, ny))
            for w, h in {(nx, ny), (ny, nx)}:
                for i0, j0 in _blocks(cells, w, h):
                    G = np.array([[P[cells[(i, j)]] for i in range(i0, i0 + w)] for j in range(j0, j0 + h)])     # rows along j, columns along i
                    if _consistent(G):
                        score = _irregularity(G)
                        if best is None or score < best[0]:
                            best = (score, G)
            if best is not None and not exhaustive:
                break
        if best is not None and not exhaustive:
            break
    if best is None:
        return none
    G = best[1]
    # a grid turned by 90 degrees in its own plane, as seen on a screen with y down: rows become columns, the handedness stays
    turns = [G, G[::-1].transpose(1, 0, 2), G[::-1, ::-1], G[:, ::-1].transpose(1, 0, 2)]
    first = min((t for t in turns if t.shape[:2] == (ny, nx)), key=lambda t: (t[0, 0, 0] + t[0, 0, 1], t[0, 0, 1]))
    return True, np.ascontiguousarray(first.reshape(nx * ny, 2))


def find_chessboard(frames, pattern_size, finder=None, **options):
    """frames: cuda u8 [B, H, W]; pattern_size (nx, ny): the INNER corners per row and column -> per frame (found, corners (nx ny, 2)
    float32).  finder: a ChessboardFinder to reuse (one is made for the frames' size otherwise); options as ChessboardFinder.corners
    takes them.  Synchronises: the grid is assembled on the host."""
    B, h, w = frames.shape[0], frames.shape[1], frames.shape[2]
    if finder is None:
        finder = ChessboardFinder(w, h, B)
    out = finder.corners(frames, **options)
    rec = records_numpy(out.records)
    counts = out.counts.cpu().numpy()
    result = []
    for b in range(B):
        r = rec[b, :counts[b, 1]]
        found, pts = assemble(np.stack([r["xf"], r["yf"]], axis=1), r["verdict"] == Q.VERDICT_OK, pattern_size)
        result.append((found, pts.astype(np.float32)))
    return result
