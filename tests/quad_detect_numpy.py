"""The quad finder's rule (include/agt_quadfind.h) stated a second time, in numpy integers and plain loops: what the device must equal
bit for bit.  It shares no code with the product and labels without scipy (tests/test_quad_detect.py holds its label image to
scipy.ndimage.label).  Rows are cut into runs of dark pixels, runs of neighbouring rows that overlap are joined in a union-find over
run numbers, and everything per component is a sort of the component's pixels."""
import numpy as np

RECORD_DTYPE = np.dtype([("label", "<i4"), ("area", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("s2", "<i8")])
FLAG_QUADS, FLAG_COMPONENTS = 1, 2
DEFAULTS = dict(min_contrast=40, min_area=24, max_area=2 ** 31 - 1, min_fill_pct=5)
MIN_EDGE_SQ = 64
DIRS = [(1024, 0), (946, 392), (724, 724), (392, 946), (0, 1024), (-392, 946), (-724, 724), (-946, 392),
        (-1024, 0), (-946, -392), (-724, -724), (-392, -946), (0, -1024), (392, -946), (724, -724), (946, -392)]


def dark_mask(img, min_contrast=40):
    """step 1 -> bool (H, W)"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    H, W = img.shape
    th, tw = H // 4, W // 4
    t = img[:4 * th, :4 * tw].astype(np.int64).reshape(th, 4, tw, 4)
    mn, mx = t.min(axis=(1, 3)), t.max(axis=(1, 3))
    MN, MX = np.empty_like(mn), np.empty_like(mx)
    for ty in range(th):
        for tx in range(tw):
            ys, xs = slice(max(ty - 1, 0), min(ty + 2, th)), slice(max(tx - 1, 0), min(tx + 2, tw))
            MN[ty, tx], MX[ty, tx] = mn[ys, xs].min(), mx[ys, xs].max()
    ty = np.minimum(np.arange(H) // 4, th - 1)[:, None]
    tx = np.minimum(np.arange(W) // 4, tw - 1)[None, :]
    lo, hi = MN[ty, tx], MX[ty, tx]
    return (hi - lo >= min_contrast) & (2 * img.astype(np.int64) < lo + hi)


def label_mask(mask):
    """step 2 -> int32 (H, W): the smallest linear index of the pixel's 4-connected component, -1 where the mask is False"""
    mask = np.asarray(mask, bool)
    H, W = mask.shape
    runs = []                     # (y, first x, last x), in linear order
    rows = []                     # per row: the numbers of its runs
    for y in range(H):
        d = np.diff(np.concatenate([[0], mask[y].astype(np.int8), [0]]))
        starts, ends = np.nonzero(d == 1)[0], np.nonzero(d == -1)[0] - 1
        rows.append(list(range(len(runs), len(runs) + len(starts))))
        runs.extend((y, int(a), int(b)) for a, b in zip(starts, ends))
    parent = list(range(len(runs)))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for y in range(1, H):
        up, cur = rows[y - 1], rows[y]
        i = j = 0
        while i < len(up) and j < len(cur):
            _, a0, a1 = runs[up[i]]
            _, b0, b1 = runs[cur[j]]
            if a0 <= b1 and b0 <= a1:               # the two runs share a column
                ra, rb = find(up[i]), find(cur[j])
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
            if a1 < b1:
                i += 1
            else:
                j += 1
    out = np.full((H, W), -1, np.int32)
    for r, (y, a, b) in enumerate(runs):
        ry, ra, _ = runs[find(r)]                   # the lowest run of the set begins at the set's smallest linear index
        out[y, a:b + 1] = ry * W + ra
    return out


def labels(img, min_contrast=40):
    return label_mask(dark_mask(img, min_contrast))


def component_sums(lab):
    """step 3 -> (labels (C,) ascending, area (C,), bbox (C, 4) x0 y0 x1 y1, support (C, 16, 2) x y)"""
    H, W = lab.shape
    ys, xs = np.nonzero(lab >= 0)
    ys, xs = ys.astype(np.int64), xs.astype(np.int64)
    l = lab[ys, xs].astype(np.int64)
    names, first, area = np.unique(l, return_index=True, return_counts=True)
    C = len(names)
    bbox, support = np.zeros((C, 4), np.int64), np.zeros((C, 16, 2), np.int64)
    if C == 0:
        return names, area, bbox, support
    idx = ys * W + xs
    for col, (key, sign) in enumerate(((xs, 1), (ys, 1), (xs, -1), (ys, -1))):
        order = np.lexsort((sign * key, l))
        bbox[:, col] = key[order][np.searchsorted(l[order], names)]
    for k, (dx, dy) in enumerate(DIRS):
        proj = xs * dx + ys * dy
        order = np.lexsort((idx, -proj, l))         # by component, then the largest projection, then the smallest index
        at = order[np.searchsorted(l[order], names)]
        support[:, k, 0], support[:, k, 1] = xs[at], ys[at]
    return names, area, bbox, support


def reduce_polygon(points):
    """the 16 support points in k order -> the vertices left (at most four), as a list of (x, y) ints"""
    pts = []
    for p in (tuple(int(v) for v in q) for q in points):
        if not pts or p != pts[-1]:
            pts.append(p)
    if len(pts) > 1 and pts[-1] == pts[0]:
        pts.pop()
    while len(pts) > 4:
        n = len(pts)
        best, at = None, 0
        for i in range(n):
            a, b, c = pts[i - 1], pts[i], pts[(i + 1) % n]
            cr = abs((b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]))
            if best is None or cr < best:
                best, at = cr, i
        del pts[at]
    return pts


def judge(area, bbox, support, W, H, min_fill_pct=5):
    """step 4 after the area limits -> (four vertices, S2) or None"""
    x0, y0, x1, y1 = (int(v) for v in bbox)
    if not (x0 > 0 and y0 > 0 and x1 < W - 1 and y1 < H - 1):
        return None
    v = reduce_polygon(support)
    if len(v) < 4:
        return None
    s2 = abs(sum(v[i][0] * v[(i + 1) % 4][1] - v[(i + 1) % 4][0] * v[i][1] for i in range(4)))
    area = int(area)
    if not (s2 > 0 and 200 * area >= min_fill_pct * s2 and 20 * area <= 11 * s2 + 400):
        return None
    cr = []
    for i in range(4):
        a, b, c = v[i], v[(i + 1) % 4], v[(i + 2) % 4]
        cr.append((b[0] - a[0]) * (c[1] - b[1]) - (b[1] - a[1]) * (c[0] - b[0]))
        if (b[0] - a[0]) ** 2 + (b[1] - a[1]) ** 2 < MIN_EDGE_SQ:
            return None
    if not (all(c > 0 for c in cr) or all(c < 0 for c in cr)):
        return None
    return v, s2


def corners(v):
    """step 5 -> f32 (4, 2)"""
    v = np.asarray(v, np.int64)
    return (v + 0.5 * np.sign(4 * v - v.sum(axis=0))).astype(np.float32)


def detect(img, max_components=4096, max_quads=512, lab=None, **options):
    """one frame -> (quads f32 (max_quads, 4, 2), records (max_quads,), counts i32 (4,)), as the device writes them"""
    o = dict(DEFAULTS, **options)
    img = np.asarray(img)
    H, W = img.shape
    if lab is None:
        lab = labels(img, o["min_contrast"])
    names, area, bbox, support = component_sums(lab)
    quads, rec, counts = np.zeros((max_quads, 4, 2), np.float32), np.zeros(max_quads, RECORD_DTYPE), np.zeros(4, np.int32)
    inside = np.nonzero((area >= o["min_area"]) & (area <= o["max_area"]))[0]
    counts[0], counts[1] = len(names), len(inside)
    if len(inside) > max_components:
        counts[3] |= FLAG_COMPONENTS
    n = 0
    for c in inside[:max_components]:
        got = judge(area[c], bbox[c], support[c], W, H, o["min_fill_pct"])
        if got is None:
            continue
        if n < max_quads:
            quads[n] = corners(got[0])
            rec[n] = (names[c], area[c], bbox[c, 0], bbox[c, 1], bbox[c, 2], bbox[c, 3], got[1])
        n += 1
    counts[2] = n
    if n > max_quads:
        counts[3] |= FLAG_QUADS
    return quads, rec, counts


def detect_batch(frames, **kw):
    out = [detect(f, **kw) for f in frames]
    return tuple(np.stack([o[i] for o in out]) for i in range(3))
