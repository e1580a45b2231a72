"""The edge refinement rule of include/agt_quadfit.h stated a second time in plain numpy FP64 (test infrastructure only; shares no
code with the product): one quad at a time, loops where the device has lanes, python floats where it has registers."""
import math

import numpy as np

OK, MASKED, DEGENERATE, SHORT, WEAK, DIVERGED = range(6)
STATUS_NAMES = ["OK", "MASKED", "DEGENERATE", "SHORT", "WEAK", "DIVERGED"]
MAX_COORD, MIN_EDGE = 1048576.0, 8.0
STATIONS, HALF_OFFSETS, MIN_USED = 16, 8, 8
RECORD_DTYPE = np.dtype([("status", "<i4"), ("passes", "<i4"), ("strength", "<f8"), ("shift", "<f8"), ("resid", "<f8")])


def strictly_convex(q):
    """+1 / -1: the common sign of the four cross products of consecutive edges, 0 when they are not of one sign or one is zero"""
    cross = []
    for i in range(4):
        j, k = (i + 1) % 4, (i + 2) % 4
        cross.append((q[j][0] - q[i][0]) * (q[k][1] - q[j][1]) - (q[j][1] - q[i][1]) * (q[k][0] - q[j][0]))
    if all(c > 0 for c in cross):
        return 1
    if all(c < 0 for c in cross):
        return -1
    return 0


def sample(frame, x, y, notes):
    """-> (inside, bilinear sample); nothing is read for a point that is not finite or whose 2 x 2 taps leave the frame"""
    h, w = frame.shape
    if not (math.isfinite(x) and math.isfinite(y)):
        return False, 0.0
    notes["frame_limit"] = min(notes["frame_limit"], abs(x), abs(x - (w - 1)), abs(y), abs(y - (h - 1)))
    fx, fy = math.floor(x), math.floor(y)
    if not (0 <= fx <= w - 2 and 0 <= fy <= h - 2):
        return False, 0.0
    a, b = x - fx, y - fy
    i00, i10, i01, i11 = float(frame[fy, fx]), float(frame[fy, fx + 1]), float(frame[fy + 1, fx]), float(frame[fy + 1, fx + 1])
    return True, (1.0 - a) * (1.0 - b) * i00 + a * (1.0 - b) * i10 + (1.0 - a) * b * i01 + a * b * i11


def fit_edge(frame, a, b, sg, range_px, notes):
    """one edge of one pass -> dict(used, strength, resid, P0, P1) (P0 / P1 None with fewer than MIN_USED used stations)"""
    dx, dy = b[0] - a[0], b[1] - a[1]
    L = math.sqrt(dx * dx + dy * dy)
    if not L > 0.0:                  # (only a later pass can get here: IEEE division gives points that are not finite, every station drops)
        return dict(used=0, strength=0.0, resid=0.0, P0=None, P1=None)
    nx, ny = sg * dy / L, sg * -dx / L
    r = min(range_px, L / 8.0)
    us, os_, gms = [], [], []
    for i in range(STATIONS):
        u = ((i + 0.5) / 16.0 - 0.5) * 0.75
        px, py = a[0] + (u + 0.5) * dx, a[1] + (u + 0.5) * dy
        dropped, Mc, Mn, gm, largest = False, 0.0, 0.0, 0.0, -math.inf
        for k in range(-HALF_OFFSETS, HALF_OFFSETS + 1):
            o = r * k / 8.0
            in1, I1 = sample(frame, px + (o + 1.0) * nx, py + (o + 1.0) * ny, notes)
            in0, I0 = sample(frame, px + (o - 1.0) * nx, py + (o - 1.0) * ny, notes)
            if not (in1 and in0):
                dropped = True
                continue
            dg = I1 - I0
            largest = max(largest, dg)
            if dg > 0.0:
                Mc += dg * dg
                Mn += dg * dg * o
                gm = max(gm, dg)
        if dropped:
            notes["dropped"] += 1
        elif largest > -1e-6:            # (with every dg clearly negative Mc is exactly 0 whoever computes it)
            notes["Mc"] = min(notes["Mc"], Mc)
        if dropped or not Mc > 0.0:
            continue
        us.append(u); os_.append(Mn / Mc); gms.append(gm)
    out = dict(used=len(us), strength=sum(gms) / len(us) if us else 0.0, resid=0.0, P0=None, P1=None)
    if len(us) < MIN_USED:
        return out
    s0, s1, s2, y0, y1 = float(len(us)), 0.0, 0.0, 0.0, 0.0
    for u, o in zip(us, os_):
        s1 += u; s2 += u * u; y0 += o; y1 += o * u
    det = s0 * s2 - s1 * s1
    alpha, beta = (s2 * y0 - s1 * y1) / det, (s0 * y1 - s1 * y0) / det
    rr = 0.0
    for u, o in zip(us, os_):
        e = o - (alpha + beta * u)
        rr += e * e
    out["resid"] = math.sqrt(rr / s0)
    t0, t1 = alpha - beta / 2.0, alpha + beta / 2.0
    out["P0"] = (a[0] + t0 * nx, a[1] + t0 * ny)
    out["P1"] = (b[0] + t1 * nx, b[1] + t1 * ny)
    return out


def intersect(l0, l1, origin):
    """the two-point cross-product form, about `origin` (the corner's place before the pass) -> (x, y) or None (DIVERGED)"""
    ox, oy = origin
    x1, y1, x2, y2 = l0["P0"][0] - ox, l0["P0"][1] - oy, l0["P1"][0] - ox, l0["P1"][1] - oy
    x3, y3, x4, y4 = l1["P0"][0] - ox, l1["P0"][1] - oy, l1["P1"][0] - ox, l1["P1"][1] - oy
    d0x, d0y, d1x, d1y = x2 - x1, y2 - y1, x4 - x3, y4 - y3
    den = d0x * d1y - d0y * d1x
    n0, n1 = math.sqrt(d0x * d0x + d0y * d0y), math.sqrt(d1x * d1x + d1y * d1y)
    if not abs(den) > 1e-12 * n0 * n1:
        return None
    c0, c1 = x1 * y2 - y1 * x2, x3 * y4 - y3 * x4
    return ox + (d0x * c1 - c0 * d1x) / den, oy + (d0y * c1 - c0 * d1y) / den


def refine_quad(frame, quad, masked=False, range_px=2.0, iters=2, min_strength=40.0):
    """-> dict(status, passes, strength, shift, resid, quad64 (4, 2) f64, quad (4, 2) f32, ok, notes).  notes: how far the decisions
    were from flipping -- frame_limit (smallest distance of a sample coordinate to 0 or size - 1), Mc (smallest sum of a station that
    was not dropped and had a dg above -1e-6) -- and how many stations were dropped, over all passes"""
    qin32 = np.asarray(quad, np.float32).reshape(4, 2)
    qin = qin32.astype(np.float64)
    notes = dict(frame_limit=np.inf, Mc=np.inf, dropped=0)
    out = dict(status=OK, passes=0, strength=0.0, shift=0.0, resid=0.0, quad64=qin.copy(), quad=qin32.copy(), ok=0, notes=notes)
    if masked:
        out["status"] = MASKED
        return out
    if not np.all(np.isfinite(qin)) or np.abs(qin).max() > MAX_COORD:
        out["status"] = DEGENERATE
        return out
    orient = strictly_convex(qin)
    if orient == 0:
        out["status"] = DEGENERATE
        return out
    for e in range(4):
        d = qin[(e + 1) % 4] - qin[e]
        if math.sqrt(d[0] * d[0] + d[1] * d[1]) < MIN_EDGE:
            out["status"] = SHORT
            return out
    shoelace = 0.0
    for e in range(4):
        f = (e + 1) % 4
        shoelace += qin[e][0] * qin[f][1] - qin[f][0] * qin[e][1]
    sg = 1.0 if shoelace > 0.0 else -1.0
    q = [(float(p[0]), float(p[1])) for p in qin]
    refused = None
    for _ in range(iters):
        edges = [fit_edge(frame, q[e], q[(e + 1) % 4], sg, range_px, notes) for e in range(4)]
        out["strength"] = min(ed["strength"] for ed in edges)
        if any(ed["used"] < MIN_USED for ed in edges):
            refused = WEAK
            break
        out["resid"] = max(ed["resid"] for ed in edges)
        new = [intersect(edges[(e + 3) % 4], edges[e], q[e]) for e in range(4)]
        if any(p is None for p in new):
            refused = DIVERGED
            break
        q = new
        out["passes"] += 1
    if refused is None:
        qa = np.array(q)
        if np.all(np.isfinite(qa)):
            out["shift"] = max(math.sqrt((qa[e][0] - qin[e][0]) ** 2 + (qa[e][1] - qin[e][1]) ** 2) for e in range(4))
        if not np.all(np.isfinite(qa)) or strictly_convex(qa) != orient or out["shift"] > 2.0 * range_px:
            refused = DIVERGED
    if refused == WEAK or out["strength"] < min_strength:
        out["status"] = WEAK
    elif refused is not None:
        out["status"] = refused
    else:
        out["quad64"] = np.array(q)
        out["quad"] = out["quad64"].astype(np.float32)
        out["ok"] = 1
    return out


def refine(frames, quads, mask=None, range_px=2.0, iters=2, min_strength=40.0):
    """frames (B, H, W) u8, quads (B, Q, 4, 2) -> list (B) of lists (Q) of refine_quad's dicts"""
    return [[refine_quad(frames[b], quads[b][q], mask is not None and mask[b][q] == 0, range_px, iters, min_strength)
             for q in range(len(quads[b]))] for b in range(len(quads))]
