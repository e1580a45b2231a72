"""Independent numpy statement of the chessboard corner finder's rule (TEST INFRASTRUCTURE).

Written from the rule in include/agt_chess.h, not from the kernels: the integer corner response, the candidates in raster order and the
FP64 saddle-point iteration with its sums in the header's fixed order.  The GPU tests hold the device to the first two byte for byte
and to the third within 1e-8 px with equal verdicts.
"""
import math

import numpy as np

RING_DX = [5, 5, 4, 2, 0, -2, -4, -5, -5, -5, -4, -2, 0, 2, 4, 5]
RING_DY = [0, 2, 4, 5, 5, 5, 4, 2, 0, -2, -4, -5, -5, -5, -4, -2]
MIN_SIZE = 11
FLAG_CANDIDATES = 1
OK, BORDER, FLAT, SHIFT = 0, 1, 2, 3
DEFAULTS = dict(min_response=200, rel_pct=10, nms=3, half=5, iters=10, max_shift=3.0, min_det=1.0)
RECORD_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("det", "<f8"), ("shift", "<f8"), ("xf", "<f4"), ("yf", "<f4"), ("verdict", "u1"),
                         ("reserved", "u1", (7,))])


def response(img):
    """u8 (H, W) -> int32 (H, W): R = 5 (SR - DR) - |5 S - 16 L| where the ring fits, 0 closer than 5 to a border"""
    a = np.asarray(img).astype(np.int64)
    H, W = a.shape
    R = np.zeros((H, W), np.int64)
    if H < MIN_SIZE or W < MIN_SIZE:
        return R.astype(np.int32)
    inner = lambda dx, dy: a[5 + dy:H - 5 + dy, 5 + dx:W - 5 + dx]
    I = [inner(dx, dy) for dx, dy in zip(RING_DX, RING_DY)]
    SR = sum(np.abs(I[k] + I[k + 8] - I[k + 4] - I[k + 12]) for k in range(4))
    DR = sum(np.abs(I[k] - I[k + 8]) for k in range(8))
    S = sum(I)
    L = inner(0, 0) + inner(-1, 0) + inner(1, 0) + inner(0, -1) + inner(0, 1)
    R[5:H - 5, 5:W - 5] = 5 * (SR - DR) - np.abs(5 * S - 16 * L)
    return R.astype(np.int32)


def candidates(R, max_candidates=1024, min_response=200, rel_pct=10, nms=3, **unused):
    """response (H, W) -> (table int32 (max_candidates, 3): x y R, counts int32 (4,): found, written, Rmax, flags)"""
    R = np.asarray(R).astype(np.int64)
    H, W = R.shape
    rmax = max(int(R.max()), 0)
    found = []
    ys, xs = np.nonzero((R >= min_response) & (100 * R >= rel_pct * rmax))
    for y, x in zip(ys.tolist(), xs.tolist()):          # (np.nonzero walks in raster order)
        r = R[y, x]
        y0, y1, x0, x1 = max(y - nms, 0), min(y + nms, H - 1), max(x - nms, 0), min(x + nms, W - 1)
        win = R[y0:y1 + 1, x0:x1 + 1].reshape(-1)
        at = (y - y0) * (x1 - x0 + 1) + (x - x0)        # raster order inside the window is raster order in the frame
        if np.all(win[:at] < r) and np.all(win[at + 1:] <= r):
            found.append((x, y, r))
    table = np.zeros((max_candidates, 3), np.int32)
    kept = found[:max_candidates]
    if kept:
        table[:len(kept)] = kept
    counts = np.array([len(found), len(kept), rmax, FLAG_CANDIDATES if len(found) > max_candidates else 0], np.int32)
    return table, counts


def weights(half):
    """(the C library's exp, as the host code of the library calls it: numpy's own exp may differ from it in the last bit)"""
    x = [(i - half) / float(half) for i in range(2 * half + 1)]
    return np.array([math.exp(-(v * v)) for v in x])


def _fixed_sum(terms):
    """terms in ascending t -> the header's sum: 64 partials, then P[l] += P[l xor m] for m = 32 .. 1"""
    P = np.zeros(64)
    for l in range(64):
        acc = 0.0
        for v in terms[l::64].tolist():
            acc = acc + v
        P[l] = acc
    idx = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        P = P + P[idx ^ m]
    return float(P[0])


def refine_one(img, seed, half=5, iters=10, max_shift=3.0, min_det=1.0, **unused):
    """one seed (x, y) on the u8 frame -> (x, y, det, shift, verdict)"""
    img = np.asarray(img)
    H, W = img.shape
    n = 2 * half + 1
    w = weights(half)
    sx, sy = float(seed[0]), float(seed[1])
    qx, qy, det, shift = sx, sy, 0.0, 0.0
    ii, jj = np.divmod(np.arange(n * n), n)
    m = w[ii] * w[jj]
    px, py = (jj - half).astype(np.float64), (ii - half).astype(np.float64)
    verdict = OK
    for _ in range(iters):
        fx, fy = np.floor(qx), np.floor(qy)
        if not (fx - (half + 1) >= 0 and fy - (half + 1) >= 0 and fx + (half + 2) <= W - 1 and fy + (half + 2) <= H - 1):
            verdict = BORDER
            break
        X, Y = int(fx), int(fy)
        a, b = qx - fx, qy - fy
        patch = img[Y - half - 1:Y + half + 3, X - half - 1:X + half + 3].astype(np.float64)
        i00, i10, i01, i11 = patch[:-1, :-1], patch[:-1, 1:], patch[1:, :-1], patch[1:, 1:]
        s = (1.0 - a) * (1.0 - b) * i00 + a * (1.0 - b) * i10 + (1.0 - a) * b * i01 + a * b * i11         # (n + 2, n + 2)
        gx = (0.5 * (s[1:-1, 2:] - s[1:-1, :-2])).reshape(-1)
        gy = (0.5 * (s[2:, 1:-1] - s[:-2, 1:-1])).reshape(-1)
        gxx, gxy, gyy = gx * gx * m, gx * gy * m, gy * gy * m
        A, Bq, Cq = _fixed_sum(gxx), _fixed_sum(gxy), _fixed_sum(gyy)
        b1, b2 = _fixed_sum(gxx * px + gxy * py), _fixed_sum(gxy * px + gyy * py)
        det = A * Cq - Bq * Bq
        if not (det > min_det) or not np.isfinite(det):
            verdict = FLAT
            break
        qx = qx + (Cq * b1 - Bq * b2) / det
        qy = qy + (A * b2 - Bq * b1) / det
        dx, dy = qx - sx, qy - sy
        shift = float(np.sqrt(dx * dx + dy * dy))
        if not shift <= max_shift:
            verdict = SHIFT
            break
    if verdict != OK:
        qx, qy = sx, sy
    return qx, qy, det, shift, verdict


def refine(img, table, counts, **options):
    """-> records (max_candidates,) structured; entries behind counts[1] zero"""
    rec = np.zeros(len(table), RECORD_DTYPE)
    n = min(max(int(counts[1]), 0), len(table))
    for k in range(n):
        x, y, det, shift, verdict = refine_one(img, table[k, :2], **options)
        rec[k] = (x, y, det, shift, np.float32(x), np.float32(y), verdict, 0)
    return rec


def corners(img, max_candidates=1024, **options):
    """stages 1 to 3 of one frame -> (table, counts, records)"""
    o = dict(DEFAULTS, **options)
    table, counts = candidates(response(img), max_candidates, **o)
    return table, counts, refine(img, table, counts, **o)


def good_points(records, counts):
    r = records[:counts[1]]
    return np.stack([r["x"], r["y"]], axis=1), r["verdict"] == OK
