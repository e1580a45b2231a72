"""CPU: the drawing library (include/agt_draw.h -> libagt_draw.so) builds, exports exactly its header, keeps its kernels out of
scratch and its survivors' list within the LDS the chunk size allows, and judges its arguments without a device; the numpy statement of
the rule (tests/overlay_numpy.py) that the GPU tests compare with has the literal properties the header promises; the `Draw` mirror
issues the reference's sequence of circle and line calls."""
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import overlay_numpy as on     # noqa: E402

WHITE = (255, 255, 255)


def test_draw_library_builds_exports_and_resources():
    import side_library
    from accurate_aprilgroup_tracking_amd import drawlib
    rows = side_library.built(drawlib, "draw")
    names = sorted(re.search(r"(draw_\w+)\(", r["name"]).group(1) for r in rows)
    assert names == ["draw_pose_lists_kernel", "draw_raster_kernel"]
    for r in rows:
        print(r)
    bad = [(r["name"], r["scratch"], r["vspill"], r["sspill"]) for r in rows if r["scratch"] != 0 or r["vspill"] != 0 or r["sspill"] != 0]
    assert not bad, bad
    # the raster's LDS: one 32-byte record per primitive of a chunk plus the per-wave survivor counts (at most one cache line);
    # the list kernel has none
    lds = {re.search(r"(draw_\w+)\(", r["name"]).group(1): r["lds"] for r in rows}
    assert 0 < lds["draw_raster_kernel"] <= drawlib.CHUNK * 32 + 64 and lds["draw_pose_lists_kernel"] == 0
    assert drawlib.lib().agt_draw_version() == drawlib.VERSION == 100
    assert drawlib.PRIM_DTYPE == on.PRIM_DTYPE and drawlib.PRIM_DTYPE.itemsize == 32
    assert (drawlib.NONE, drawlib.DISC, drawlib.SEGMENT) == (on.NONE, on.DISC, on.SEGMENT)
    assert (drawlib.MAX_COORD, drawlib.MAX_SIZE) == (on.MAX_COORD, on.MAX_SIZE) == (32767, 64)
    header = open(os.path.join(ROOT, "include", "agt_draw.h")).read()
    for name, value in (("CHUNK", drawlib.CHUNK), ("MAX_COORD", 32767), ("MAX_SIZE", 64), ("MAX_PRIMS", drawlib.MAX_PRIMS),
                        ("MAX_TOTAL", drawlib.MAX_TOTAL), ("MAX_POINTS", drawlib.MAX_POINTS), ("MAX_SIZE_PX", drawlib.MAX_SIZE_PX),
                        ("CLEAR", drawlib.CLEAR), ("VERSION", 100)):
        assert re.search(r"#define AGT_DRAW_%s\s+%d\b" % (name, value), header), name


def test_argument_errors_need_no_device():
    """no pointer is followed: every refusal comes before device work.  (A call with good arguments would launch: none is made.)"""
    from accurate_aprilgroup_tracking_amd import drawlib as D
    L = D.lib()
    good = dict(frames=64, pitch=1280 * 3, frame_stride=1280 * 3 * 720, width=1280, height=720, channels=3, B=2, prims=64, P=48, flags=0)

    def raster(**kw):
        a = dict(good, **kw)
        return L.agt_draw_raster(None, a["frames"], a["pitch"], a["frame_stride"], a["width"], a["height"], a["channels"], a["B"], a["prims"],
                                 a["P"], a["flags"])
    for kw in (dict(frames=None), dict(prims=None), dict(width=0), dict(height=0), dict(width=D.MAX_SIZE_PX + 1, pitch=1 << 20, frame_stride=1 << 40),
               dict(height=D.MAX_SIZE_PX + 1, frame_stride=1 << 40), dict(channels=2), dict(channels=0), dict(channels=4), dict(pitch=1280 * 3 - 1),
               dict(channels=1, pitch=1279), dict(frame_stride=1280 * 3 * 720 - 1), dict(P=-1), dict(P=D.MAX_PRIMS + 1), dict(B=0), dict(B=-1),
               dict(B=257, P=4096, frame_stride=1 << 40), dict(B=1 << 20, P=2, frame_stride=1 << 40), dict(flags=2), dict(flags=3)):
        assert raster(**kw) == D.ERR_ARG, kw
    # P = 0 without CLEAR is nothing to do: accepted with a NULL list, and nothing is launched
    assert raster(prims=None, P=0) == 0

    fine = dict(points=64, dtype=D.F64, n=48, B=2, gate=None, gate_stride=0, width=1280, height=720, cpt=4, radius=5, thickness=5,
                dot=0xFF0000, line=0xFFFFFF, dots=64, outline=64)

    def lists(**kw):
        a = dict(fine, **kw)
        return L.agt_draw_pose_lists(None, a["points"], a["dtype"], a["n"], a["B"], a["gate"], a["gate_stride"], a["width"], a["height"], a["cpt"],
                                     a["radius"], a["thickness"], a["dot"], a["line"], a["dots"], a["outline"])
    for kw in (dict(points=None), dict(dots=None), dict(outline=None), dict(dtype=2), dict(dtype=-1), dict(n=0), dict(n=46), dict(n=47), dict(n=2),
               dict(n=D.MAX_POINTS + 4), dict(B=0), dict(B=-1), dict(B=(1 << 20) // 48 + 1), dict(width=0), dict(height=0), dict(width=D.MAX_SIZE_PX + 1),
               dict(height=D.MAX_SIZE_PX + 1), dict(cpt=3), dict(cpt=8), dict(radius=-1), dict(radius=65), dict(thickness=-1), dict(thickness=65),
               dict(gate=64, gate_stride=0), dict(dot=1 << 24), dict(line=1 << 31)):
        assert lists(**kw) == D.ERR_ARG, kw
    with pytest.raises(D.DrawError, match="AGT_DRAW_ERR_ARG"):
        D.raster(None, 64, 1280 * 3, 0, 1280, 720, 2, 1, 64, 4)
    with pytest.raises(D.DrawError, match="AGT_DRAW_ERR_ARG"):
        D.pose_lists(None, 64, D.F32, 6, 1, None, 0, 1280, 720, 4, 5, 5, 0, 0, 64, 64)


def test_missing_library_raises(monkeypatch):
    from accurate_aprilgroup_tracking_amd import drawlib
    monkeypatch.setattr(drawlib, "_lib", None)
    monkeypatch.setattr(drawlib, "LIB_PATH", "/nonexistent/libagt_draw.so")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        drawlib.lib()


# ---- literals of the numpy statement
def test_disc_of_radius_5_has_the_stated_rows():
    m = on.coverage(on.disc(20, 20, 5, WHITE), 41, 41)
    rows = m.sum(axis=1)
    assert rows[rows > 0].tolist() == [5, 7, 9, 11, 11, 11, 11, 11, 9, 7, 5] and m.sum() == 97
    assert np.array_equal(m, m.T) and np.array_equal(m, m[::-1]) and m[15:26, 15:26].sum() == 97
    assert on.coverage(on.disc(3, 4, 0, WHITE), 9, 9).sum() == 1 and on.coverage(on.disc(3, 4, 0, WHITE), 9, 9)[4, 3]


def test_zero_length_segment_is_its_round_cap():
    m = on.coverage(on.segment(10, 10, 10, 10, 5, WHITE), 21, 21)
    assert m.sum() == 21
    assert m.sum(axis=1)[8:13].tolist() == [3, 5, 5, 5, 3]


def test_horizontal_segment_rows_odd_and_even_thickness():
    for T, rows in ((5, 5), (1, 1), (3, 3), (2, 3), (4, 5), (64, 65)):
        m = on.coverage(on.segment(100, 100, 140, 100, T, WHITE), 240, 200)
        assert np.flatnonzero(m.any(axis=1)).size == rows, T
        assert m[:, 120].sum() == rows
        assert np.array_equal(on.coverage(on.segment(100, 100, 100, 140, T, WHITE), 200, 240), m.T[:240, :200]), T


def test_thickness_1_leaves_no_gap_in_any_direction():
    """every direction of a 40 x 40 grid: the painted pixels of a 1-px segment form one 8-connected chain from end to end, and every
    row (column) between the ends of a steep (flat) segment holds a pixel"""
    c = 45
    for dx in range(-40, 41):
        for dy in range(-40, 41):
            if max(abs(dx), abs(dy)) != 40:
                continue                        # (the border of the grid gives every direction)
            m = on.coverage(on.segment(c, c, c + dx, c + dy, 1, WHITE), 2 * c + 1, 2 * c + 1)
            assert m[c, c] and m[c + dy, c + dx]
            ys, xs = np.nonzero(m)
            if abs(dy) >= abs(dx):
                assert set(ys) == set(range(min(c, c + dy), max(c, c + dy) + 1)), (dx, dy)
            if abs(dx) >= abs(dy):
                assert set(xs) == set(range(min(c, c + dx), max(c, c + dx) + 1)), (dx, dy)
            # 8-connected: walk from one end
            todo, seen = [(c, c)], {(c, c)}
            pix = set(zip(ys.tolist(), xs.tolist()))
            while todo:
                y, x = todo.pop()
                for ny in (y - 1, y, y + 1):
                    for nx in (x - 1, x, x + 1):
                        if (ny, nx) in pix and (ny, nx) not in seen:
                            seen.add((ny, nx)); todo.append((ny, nx))
            assert seen == pix, (dx, dy)


def test_invalid_primitives_paint_nothing_and_the_cross_term_is_exact():
    for p in (on.prim(3, 5, 5, 5, 5, 2, WHITE), on.prim(-1, 5, 5, 5, 5, 2, WHITE), on.prim(on.NONE, 5, 5, 5, 5, 2, WHITE),
              on.disc(32768, 5, 2, WHITE), on.segment(5, 5, 5, -32768, 2, WHITE), on.segment(1 << 30, 5, 5, 5, 2, WHITE),
              on.disc(5, 5, -1, WHITE), on.disc(5, 5, 65, WHITE)):
        assert not on.coverage(p, 16, 16).any()
    # the longest segment there is: the squared cross product passes 2^64, the verdicts are those of exact rational geometry
    a, b = (-32767, -32767), (32767, 32766)
    for T in (1, 64):
        m = on.coverage(on.segment(a[0], a[1], b[0], b[1], T, WHITE), 129, 65)
        dx, dy = b[0] - a[0], b[1] - a[1]
        L = math.hypot(dx, dy)
        for y in range(65):
            for x in range(0, 129, 7):
                d = abs(dx * (y - a[1]) - dy * (x - a[0])) / L
                if abs(d - T / 2) > 1e-6:
                    assert m[y, x] == (d < T / 2), (T, x, y)
        assert m.any() and not m.all()


def test_pose_lists_rounding_and_frame_rule():
    w, h = 70, 37
    pts = np.array([[[0.5, 1.5], [2.5, -0.4], [w - 0.5, 3.0], [3.0, h - 0.5]],
                    [[10.0, 10.0], [20.9, 10.0], [20.0, 20.0], [10.0, 20.9]]])
    dots, outline = on.pose_lists(pts.reshape(1, 8, 2), w, h)
    d = dots[0]
    assert (d["x0"][0], d["y0"][0]) == (0, 2) and (d["x0"][1], d["y0"][1]) == (2, 0)
    assert d["kind"][2] == on.NONE                      # 69.5 rounds to 70: outside
    assert (d["kind"][3], d["y0"][3]) == (on.DISC, 36)    # 36.5 rounds to 36: inside
    o = outline[0]
    assert o["kind"][:4].tolist() == [on.SEGMENT] * 4     # int(-0.4) = 0, int(69.5) = 69: inside
    assert [(int(s["x0"]), int(s["y0"]), int(s["x1"]), int(s["y1"])) for s in o[4:]] == [(10, 10, 20, 10), (20, 10, 20, 20), (20, 20, 10, 20), (10, 20, 10, 10)]
    gated = on.pose_lists(pts.reshape(1, 8, 2), w, h, gate=np.array([np.nan]))
    assert not gated[0]["kind"].any() and not gated[1]["kind"].any() and gated[0].tobytes() == bytes(32 * 8)


# ---- the Draw mirror
class RecordingCV:
    def __init__(self):
        self.calls = []

    def circle(self, img, center, radius, color, thickness=None):
        self.calls.append(("circle", id(img), tuple(center), radius, tuple(color), thickness))

    def line(self, img, pt1, pt2, color, thickness=None, lineType=None):
        self.calls.append(("line", id(img), tuple(pt1), tuple(pt2), tuple(color), thickness, lineType))


def test_draw_mirror_issues_the_reference_call_sequence():
    from accurate_aprilgroup_tracking_amd.draw import Draw
    cv = RecordingCV()
    img, frame = np.zeros((720, 1280, 3), np.uint8), np.zeros((720, 1280, 3), np.uint8)
    # two tags; the second has one point left of the frame (its dot and its whole outline are skipped), one value rounds half to even
    pts = np.array([[[100.5, 200.4]], [[150.6, 200.5]], [[150.2, 250.9]], [[100.9, 250.1]],
                    [[-3.0, 300.0]], [[40.0, 300.0]], [[40.0, 340.0]], [[2.0, 340.0]]])
    Draw(None, cv=cv).draw_squares_and_3d_pts(img, frame, pts)
    red, T, AA = (0, 0, 255), 5, 16
    expect = [("circle", id(img), c, 5, red, -1) for c in ((100, 200), (151, 200), (150, 251), (101, 250), (40, 300), (40, 340), (2, 340))]
    q = [(100, 200), (150, 200), (150, 250), (100, 250)]
    expect += [("line", id(frame), q[k], q[(k + 1) % 4], WHITE, T, AA) for k in range(4)]
    assert cv.calls == expect
    assert all(type(v) is int for c in cv.calls for v in c[2])
    with pytest.raises(ValueError, match="Image points are empty"):
        Draw(None, cv=cv).draw_squares_and_3d_pts(img, frame, np.array([[[0.0, 5.0]], [[1.0, 1.0]], [[2.0, 2.0]], [[3.0, 3.0]]]))

    cv.calls.clear()
    box = np.arange(16, dtype=np.float64).reshape(8, 1, 2) * 10 + 5.4
    Draw(None, cv=cv).draw_boxes(img, box)
    ip = [(int(round(x)), int(round(y))) for x, y in box.reshape(-1, 2)]
    edges = [(0, 1), (1, 2), (2, 3), (3, 0), (0, 4), (1, 5), (2, 6), (3, 7), (4, 5), (5, 6), (6, 7), (7, 4)]
    assert cv.calls == [("line", id(img), ip[i], ip[j], (0, 255, 0), 1, 16) for i, j in edges]

    cv.calls.clear()

    class Det:
        corners = np.array([[10.9, 10.2], [50.1, 10.9], [50.5, 50.5], [10.0, 50.0]])
        center = np.array([30.7, 30.2])
        tag_id = 3
    Draw(None, cv=cv).draw_corners(img, Det)
    c = [(10, 10), (50, 10), (50, 50), (10, 50)]
    assert cv.calls == [("line", id(img), c[k], c[(k + 1) % 4], (0, 255, 0), 5, None) for k in range(4)] + [("circle", id(img), (30, 30), 5, (0, 255, 255), -1)]
