"""The tag decode rule of include/agt_tagcode.h stated a second time in plain numpy FP64 (test infrastructure only; shares no code
with the product): one quad at a time, loops where the device has lanes, np.linalg.solve where it has closed forms."""
import numpy as np

OK, MASKED, DEGENERATE, OUTSIDE, INVERTED, NO_MATCH, LOW_MARGIN = range(7)
MAX_COORD = 1048576.0
SQUARE = np.array([[-1.0, -1.0], [-1.0, 1.0], [1.0, 1.0], [1.0, -1.0]])      # (u, v) of q0..q3
CELLS = [(r, c) for r in range(-1, 9) for c in range(-1, 9)]
RING = [(r, c) for r, c in CELLS if r in (-1, 8) or c in (-1, 8)]
BORDER = [(r, c) for r, c in CELLS if (r, c) not in RING and (r in (0, 7) or c in (0, 7))]
PAYLOAD = [(r, c) for r in range(1, 7) for c in range(1, 7)]
assert (len(RING), len(BORDER), len(PAYLOAD)) == (36, 28, 36)
RECORD_DTYPE = np.dtype([("id", "<i4"), ("hamming", "<i4"), ("rot", "<i4"), ("status", "<i4"), ("margin", "<f8"), ("contrast", "<f8"),
                         ("word", "<u8")])


def centre(r, c):
    return (2 * c + 1) / 8.0 - 1.0, (2 * r + 1) / 8.0 - 1.0


def word_of(bits):
    """(6, 6) bits -> the word: bit 35 - (6 r + c) is row r, column c"""
    w = 0
    for r in range(6):
        for c in range(6):
            if bits[r][c]:
                w |= 1 << (35 - (6 * r + c))
    return w


def bits_of(word):
    return np.array([[(int(word) >> (35 - (6 * r + c))) & 1 for c in range(6)] for r in range(6)], np.uint8)


def candidates(codes):
    """[(i, k, word of np.rot90(bits_i, -k))] in tie order"""
    return [(i, k, word_of(np.rot90(bits_of(code), -k))) for i, code in enumerate(codes) for k in range(4)]


def homography(quad):
    """square -> quad by the 8 x 8 linear system, solved about q0 so that the unknowns are of the quad's size, then moved back"""
    q = np.asarray(quad, np.float64)
    p = q - q[0]
    A, rhs = [], []
    for (u, v), (x, y) in zip(SQUARE, p):
        A.append([u, v, 1, 0, 0, 0, -u * x, -v * x]); rhs.append(x)
        A.append([0, 0, 0, u, v, 1, -u * y, -v * y]); rhs.append(y)
    h = np.linalg.solve(np.array(A), np.array(rhs))
    Hc = np.append(h, 1.0).reshape(3, 3)
    T = np.array([[1.0, 0.0, q[0, 0]], [0.0, 1.0, q[0, 1]], [0.0, 0.0, 1.0]])
    return T @ Hc


def plane(cells, values):
    """least-squares a u + b v + c through the samples: 3 x 3 normal equations"""
    A = np.array([[*centre(r, c), 1.0] for r, c in cells])
    return np.linalg.solve(A.T @ A, A.T @ np.asarray(values))


def decode_quad(frame, quad, cand, masked=False, expected=None, max_hamming=2, min_margin=0.0):
    """-> dict(id, hamming, rot, status, margin, contrast, word, ok, H (3, 3), d: {(r, c): I - thr} or None)"""
    out = dict(id=-1, hamming=-1, rot=-1, status=OK, margin=0.0, contrast=0.0, word=0, ok=0, H=np.zeros((3, 3)), d=None)
    if masked:
        out["status"] = MASKED
        return out
    q = np.asarray(quad, np.float32).astype(np.float64).reshape(4, 2)
    if not np.all(np.isfinite(q)) or np.abs(q).max() > MAX_COORD:
        out["status"] = DEGENERATE
        return out
    cross = []
    for i in range(4):
        e0, e1 = q[(i + 1) % 4] - q[i], q[(i + 2) % 4] - q[(i + 1) % 4]
        cross.append(e0[0] * e1[1] - e0[1] * e1[0])
    if not (all(c > 0 for c in cross) or all(c < 0 for c in cross)):
        out["status"] = DEGENERATE
        return out
    H = homography(q)
    out["H"] = H
    h, w = frame.shape
    pts = {}
    with np.errstate(all="ignore"):
        for r, c in CELLS:
            u, v = centre(r, c)
            den = H[2, 0] * u + H[2, 1] * v + H[2, 2]
            x, y = (H[0, 0] * u + H[0, 1] * v + H[0, 2]) / den, (H[1, 0] * u + H[1, 1] * v + H[1, 2]) / den
            if not np.isfinite(den) or den == 0.0 or not np.isfinite(x) or not np.isfinite(y):
                out["status"] = DEGENERATE
                return out
            pts[(r, c)] = (x, y)
    for x, y in pts.values():
        if not (0 <= np.floor(x) <= w - 2 and 0 <= np.floor(y) <= h - 2):
            out["status"] = OUTSIDE
            return out
    I = {}
    for rc, (x, y) in pts.items():
        x0, y0 = int(np.floor(x)), int(np.floor(y))
        a, b = x - x0, y - y0
        f = frame[y0:y0 + 2, x0:x0 + 2].astype(np.float64)
        I[rc] = (1 - a) * (1 - b) * f[0, 0] + a * (1 - b) * f[0, 1] + (1 - a) * b * f[1, 0] + a * b * f[1, 1]
    W, Bk = plane(RING, [I[rc] for rc in RING]), plane(BORDER, [I[rc] for rc in BORDER])
    d, gap = {}, []
    for r, c in PAYLOAD:
        u, v = centre(r, c)
        wv, bv = W @ [u, v, 1.0], Bk @ [u, v, 1.0]
        d[(r, c)] = I[(r, c)] - (wv + bv) / 2
        gap.append(wv - bv)
    contrast = float(np.mean(gap))
    if contrast <= 0:
        out["status"] = INVERTED
        return out
    ones = [v for v in d.values() if v > 0]
    zeros = [-v for v in d.values() if not v > 0]
    margin = min(np.mean(ones) if ones else 0.0, np.mean(zeros) if zeros else 0.0)
    word = word_of([[d[(r, c)] > 0 for c in range(1, 7)] for r in range(1, 7)])
    best = None
    for i, k, cw in cand:
        ham = bin(word ^ cw).count("1")
        if best is None or ham < best[0]:
            best = (ham, i, k)
    out.update(hamming=best[0], id=best[1], rot=best[2], margin=float(margin), contrast=contrast, word=word, d=d)
    if best[0] > max_hamming:
        out["status"] = NO_MATCH
    elif margin < min_margin:
        out["status"] = LOW_MARGIN
    out["ok"] = int(out["status"] == OK and (expected is None or (out["id"] == expected and out["rot"] == 0)))
    return out


def decode(frames, quads, codes, mask=None, expected=None, max_hamming=2, min_margin=0.0):
    """frames (B, H, W) u8, quads (B, Q, 4, 2) -> list (B) of lists (Q) of decode_quad's dicts"""
    cand = candidates(codes)
    return [[decode_quad(frames[b], quads[b][q], cand, mask is not None and mask[b][q] == 0, None if expected is None else int(expected[q]),
                         max_hamming, min_margin) for q in range(len(quads[b]))] for b in range(len(quads))]
