"""CPU: the quad finder library (include/agt_quadfind.h -> libagt_quadfind.so) builds, exports exactly its header and keeps every
kernel out of scratch; the numpy statement of its rule (tests/quad_detect_numpy.py), which the GPU tests hold the device to bit for
bit, labels as scipy does and finds every front tag of the rendered scenes well enough for the refinement; the Python doors refuse bad
arguments without a device."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import quad_detect_numpy as qd      # noqa: E402
import quad_detect_scenes as S      # noqa: E402
import quad_refine_numpy as qn      # noqa: E402
import tag_decode_scenes as ts      # noqa: E402

KERNELS = ["qf_emit", "qf_flatten_area", "qf_label_tiles", "qf_merge_borders", "qf_quads", "qf_root_assign", "qf_root_count", "qf_root_scan",
           "qf_support", "qf_tile_minmax", "qf_tile_neigh"]


# ---- A: the library

def test_quadfind_library_builds_exports_and_resources():
    import side_library
    from accurate_aprilgroup_tracking_amd import quadfindlib
    rows = side_library.built(quadfindlib, "quadfind")
    assert sorted(re.search(r"(qf_\w+)\(", r["name"]).group(1) for r in rows) == KERNELS
    for r in rows:
        print(r)
    bad = [(r["name"], r["scratch"], r["vspill"], r["sspill"]) for r in rows if r["scratch"] != 0 or r["vspill"] != 0 or r["sspill"] != 0]
    assert not bad, bad
    # the labelling tile and the vertex lists are all the LDS there is; no kernel is short of registers for full occupancy
    assert max(r["lds"] for r in rows) <= 8192 and max(r["vgpr"] for r in rows) <= 64
    assert quadfindlib.lib().agt_quadfind_version() == quadfindlib.VERSION == 100
    assert quadfindlib.RECORD_DTYPE == qd.RECORD_DTYPE and quadfindlib.DEFAULTS == qd.DEFAULTS
    assert (quadfindlib.FLAG_QUADS, quadfindlib.FLAG_COMPONENTS) == (qd.FLAG_QUADS, qd.FLAG_COMPONENTS)


def test_header_states_the_directions_and_limits_the_modules_use():
    from accurate_aprilgroup_tracking_amd import quadfindlib as Q
    text = open(os.path.join(ROOT, "include", "agt_quadfind.h")).read()
    want = {k: np.rint(1024 * f(2 * np.pi * np.arange(16) / 16)).astype(int) for k, f in (("dx", np.cos), ("dy", np.sin))}
    for k, col in (("dx", 0), ("dy", 1)):
        stated = [int(v) for v in re.search(r"%s = ((?:-?\d+ ?){16})" % k, text).group(1).split()]
        assert stated == list(want[k]) == [d[col] for d in qd.DIRS]
    defines = dict(re.findall(r"#define AGT_QUADFIND_(\w+)\s+\(?(-?\d+)\)?", text))
    assert (int(defines["MIN_SIZE"]), int(defines["MAX_SIZE"]), int(defines["MAX_BATCH"]), int(defines["MAX_COMPONENTS"]), int(defines["MAX_QUADS"])) == \
        (Q.MIN_SIZE, Q.MAX_SIZE, Q.MAX_BATCH, Q.MAX_COMPONENTS, Q.MAX_QUADS)
    assert (int(defines["ERR_ARG"]), int(defines["ERR_ALLOC"]), int(defines["ERR_HIP"])) == (Q.ERR_ARG, Q.ERR_ALLOC, Q.ERR_HIP)
    assert (int(defines["FLAG_QUADS"]), int(defines["FLAG_COMPONENTS"])) == (Q.FLAG_QUADS, Q.FLAG_COMPONENTS)
    assert qd.MIN_EDGE_SQ == qn.MIN_EDGE ** 2


def test_missing_library_raises(monkeypatch):
    from accurate_aprilgroup_tracking_amd import quadfindlib
    monkeypatch.setattr(quadfindlib, "_lib", None)
    monkeypatch.setattr(quadfindlib, "LIB_PATH", "/nonexistent/libagt_quadfind.so")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        quadfindlib.lib()


# ---- B: the statement labels as scipy does

@pytest.mark.parametrize("w,h", S.LABEL_SIZES + [(257, 129)])
def test_numpy_labels_equal_scipy_on_the_patterns(w, h):
    frames, masks, labels = S.pattern_frames(w, h)
    for p, f, m, l in zip(S.PATTERNS, frames, masks, labels):
        dark = qd.dark_mask(f)
        assert np.array_equal(dark, m), "%s: drawn 0 / 255 the dark mask is the pattern" % p.__name__
        assert l.dtype == np.int32 and np.array_equal(l, S.scipy_labels(dark)), p.__name__
        roots = np.unique(l[l >= 0])
        assert np.all(l.reshape(-1)[roots] == roots), "a label is the index of one of the component's own pixels"
    count = {p.__name__: len(np.unique(l[l >= 0])) for p, l in zip(S.PATTERNS, labels)}
    assert (count["spiral"], count["comb"], count["u_shape"], count["serpentine"], count["diagonal_blobs"], count["uniform"]) == (1, 1, 1, 1, 2, 0)
    assert count["checkerboard"] == int(masks[S.PATTERNS.index(S.checkerboard)].sum())


@pytest.mark.parametrize("name,k", S.SCENE_FRAMES)
def test_numpy_labels_equal_scipy_on_the_scenes(name, k):
    img = ts.sequence(name).frame(k)
    dark = qd.dark_mask(img)
    assert np.array_equal(qd.label_mask(dark), S.scipy_labels(dark))


def test_dark_mask_by_plain_loops():
    """the vectorised mask of the statement against the rule read word by word, on a frame whose sizes are no multiples of four"""
    img = ts.sequence("small").frame(0)[100:147, 200:261]
    H, W = img.shape
    th, tw = H // 4, W // 4
    want = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            ty, tx = min(y // 4, th - 1), min(x // 4, tw - 1)
            y0, y1, x0, x1 = max(ty - 1, 0), min(ty + 1, th - 1), max(tx - 1, 0), min(tx + 1, tw - 1)
            block = img[4 * y0:4 * y1 + 4, 4 * x0:4 * x1 + 4].astype(int)
            want[y, x] = block.max() - block.min() >= 40 and 2 * int(img[y, x]) < block.min() + block.max()
    assert want.any() and not want.all() and np.array_equal(qd.dark_mask(img), want)


def test_component_sums_by_plain_loops():
    lab = qd.labels(ts.sequence("small").frame(0)[180:300, 250:420])
    H, W = lab.shape
    names, area, bbox, support = qd.component_sums(lab)
    assert len(names) > 20 and np.all(np.diff(names) > 0)
    for c in range(0, len(names), 7):
        ys, xs = np.nonzero(lab == names[c])
        assert area[c] == len(ys) and list(bbox[c]) == [xs.min(), ys.min(), xs.max(), ys.max()]
        for k, (dx, dy) in enumerate(qd.DIRS):
            best = None
            for x, y in zip(xs.tolist(), ys.tolist()):          # (row-major: the first of equals has the smallest index)
                if best is None or x * dx + y * dy > best[0]:
                    best = (x * dx + y * dy, x, y)
            assert tuple(support[c, k]) == best[1:]


def test_polygon_reduction_and_filters_at_their_edges():
    sq = [(10, 10), (30, 10), (30, 30), (10, 30)]
    # 16 support points of an axis-aligned square: each corner several times over
    pts = [sq[1]] * 1 + [sq[2]] * 4 + [sq[3]] * 4 + [sq[0]] * 4 + [sq[1]] * 3
    assert qd.reduce_polygon(pts) == [sq[1], sq[2], sq[3], sq[0]]
    # a fifth vertex a hair off an edge goes first; of two equal triangles the one lower in the list
    assert qd.reduce_polygon([sq[0], (20, 9), sq[1], sq[2], sq[3]]) == sq
    assert qd.reduce_polygon([sq[0], (20, 9), sq[1], (31, 20), sq[2], sq[3]]) == sq
    assert qd.reduce_polygon([(0, 0), (10, 0), (20, 0), (20, 10), (20, 20), (0, 20)]) == [(0, 0), (20, 0), (20, 20), (0, 20)]
    assert qd.reduce_polygon([(5, 5)] * 16) == [(5, 5)] and qd.reduce_polygon([(0, 0)] * 8 + [(9, 9)] * 8) == [(0, 0), (9, 9)]
    sup = np.array(pts)
    s2 = 2 * 20 * 20
    assert qd.judge(441, (10, 10, 30, 30), sup, 64, 48)[1] == s2
    for bbox in ((0, 10, 30, 30), (10, 0, 30, 30), (10, 10, 63, 30), (10, 10, 30, 47)):
        assert qd.judge(441, bbox, sup, 64, 48) is None
    # the fill limits: 200 area >= pct S2, 20 area <= 11 S2 + 400
    assert qd.judge(20, (10, 10, 30, 30), sup, 64, 48, min_fill_pct=5) is not None and qd.judge(19, (10, 10, 30, 30), sup, 64, 48, min_fill_pct=5) is None
    assert qd.judge(460, (10, 10, 30, 30), sup, 64, 48) is not None and qd.judge(461, (10, 10, 30, 30), sup, 64, 48) is None
    # an edge of 8 px is kept, one of under 8 is not; a triangle is none
    small = np.array([(10, 10)] * 4 + [(18, 10)] * 4 + [(18, 18)] * 4 + [(10, 18)] * 4)
    assert qd.judge(64, (10, 10, 18, 18), small, 64, 48) is not None
    assert qd.judge(64, (10, 10, 17, 18), np.where(small == 18, [17, 18], small), 64, 48) is None
    assert qd.judge(100, (10, 10, 30, 30), np.array([sq[0]] * 6 + [sq[1]] * 5 + [sq[2]] * 5), 64, 48) is None
    c = qd.corners(sq)
    assert c.dtype == np.float32 and c.tolist() == [[9.5, 9.5], [30.5, 9.5], [30.5, 30.5], [9.5, 30.5]]
    assert qd.corners([(0, 10), (10, 0), (20, 10), (10, 20)]).tolist() == [[-0.5, 10.0], [10.0, -0.5], [20.5, 10.0], [10.0, 20.5]]


# ---- C: what the statement alone must deliver

@pytest.mark.parametrize("name,k", S.SCENE_FRAMES)
def test_numpy_statement_finds_every_front_tag(name, k):
    """Every tag seen at under 60 degrees has a candidate whose corners are within 3.0 px under some rotation or orientation (the
    measure is the one of the issue's table, the largest coordinate difference: it reproduces its 1.83 / 2.68 / 2.17 px), that
    candidate refines to OK with quad_refine_numpy's defaults and lands within 0.35 px (corner distance) of the truth; fewer than 512
    candidates per frame."""
    r = S.numpy_chain(name, k)
    print("%s %d: counts %s, %d front tags, worst raw %.2f px (distance %.2f), worst refined %.3f px" %
          (name, k, r["counts"], len(r["front"]), r["raw"].max(), r["raw_l2"].max(), r["refined"].max()))
    assert len(r["front"]) >= 3
    assert r["counts"][2] < S.MAX_CANDIDATES and r["counts"][3] == 0
    assert r["raw"].max() <= S.RAW_PX
    assert np.all(r["status"] == qn.OK)
    assert r["refined"].max() <= S.REFINED_PX
    assert len(set(r["candidate"])) == len(r["front"]), "one candidate per tag"
    n = int(r["counts"][2])
    assert np.all(np.diff(r["records"]["label"][:n]) > 0) and not r["records"][n:].tobytes().strip(b"\0") and not r["quads"][n:].any()


def test_numpy_statement_finds_all_visible_tags_of_dense():
    seq = ts.sequence("dense")
    quads, rec, counts = qd.detect(seq.frame(0))
    truth = ts.quads(seq, 0).astype(np.float64)
    found = [t for t in range(len(truth)) if min(S.match_error(q, truth[t])[0] for q in quads[:counts[2]]) <= S.RAW_PX]
    visible = np.nonzero(ts.view_cosines(seq, 0) > 0.0)[0]
    print("dense 0: %d of %d visible tags found" % (len(set(found) & set(visible)), len(visible)))
    assert set(ts.front_tags(seq, 0)) <= set(found)


@pytest.mark.parametrize("i", range(len(S.SINGLE_QUADS)))
def test_numpy_statement_on_single_quads(i):
    """the quads of the issue's table: one candidate each (the 150-px one has a hollow mask).  The bound on the raw corners: the pixel
    that holds a right-angled vertex is covered by under a half and so is not dark, the extreme dark pixel's centre lies within
    1.5 px of the vertex on each axis, and the half-pixel step outwards can add to that: 2 px."""
    frame, truth = S.single_quad(i)
    quads, rec, counts = qd.detect(frame)
    assert counts[2] == 1 and counts[3] == 0
    err = S.match_error(quads[0], truth)[0]
    print(S.SINGLE_QUADS[i], "raw corner error %.2f px, area %d, S2 %d" % (err, rec[0]["area"], rec[0]["s2"]))
    assert err <= 2.0
    shoelace = lambda q: sum(q[e][0] * q[(e + 1) % 4][1] - q[(e + 1) % 4][0] * q[e][1] for e in range(4))
    assert shoelace(quads[0]) > 0 and shoelace(truth) > 0, "the vertices run from +x towards +y: clockwise on the screen"
    if i == 4:
        assert rec[0]["area"] < 0.5 * rec[0]["s2"] / 2, "hollow"


def test_numpy_statement_at_the_frame_borders():
    for kind, frame, truth in S.border_quads():
        quads, rec, counts = qd.detect(frame)
        assert counts[2] == (1 if kind == "inside" else 0), kind
        if kind == "inside":
            assert S.match_error(quads[0], truth)[0] <= 2.0 and min(rec[0]["x0"], rec[0]["y0"], 199 - rec[0]["x1"], 159 - rec[0]["y1"]) in (1, 2)


def test_numpy_statement_caps():
    """max_quads and max_components keep the first entries in label order and change none of them"""
    img = ts.sequence("small").frame(0)
    full = qd.detect(img)
    n = int(full[2][2])
    few = qd.detect(img, max_quads=5)
    assert few[2].tolist() == [full[2][0], full[2][1], n, qd.FLAG_QUADS] and few[0].tobytes() == full[0][:5].tobytes() and few[1].tobytes() == full[1][:5].tobytes()
    names, area, _, _ = qd.component_sums(qd.labels(img))
    seventh = names[(area >= 24)][6]
    cut = qd.detect(img, max_components=7)
    m = int((full[1]["label"][:n] <= seventh).sum())
    assert cut[2].tolist() == [full[2][0], full[2][1], m, qd.FLAG_COMPONENTS] and cut[1][:m].tobytes() == full[1][:m].tobytes() and not cut[0][m:].any()


# ---- D: refusals that need no device

def test_python_refusals_need_no_device():
    import torch
    from accurate_aprilgroup_tracking_amd import quad_detect, quadfindlib as Q, tag_detect, tag_decode
    for kw in (dict(width=7), dict(height=7), dict(width=Q.MAX_SIZE + 1), dict(max_batch=0), dict(max_batch=Q.MAX_BATCH + 1), dict(max_components=0),
               dict(max_quads=0), dict(max_quads=9, max_components=8), dict(max_components=Q.MAX_COMPONENTS + 1)):
        with pytest.raises(Q.QuadFindError, match="AGT_QUADFIND_ERR_ARG"):
            quad_detect.QuadDetector(**dict(dict(width=64, height=48), **kw))
    det = quad_detect.QuadDetector(64, 48, max_batch=2)
    with pytest.raises(TypeError, match="min_contrst"):
        det.detect(torch.zeros((1, 48, 64), dtype=torch.uint8), min_contrst=3)
    with pytest.raises(Q.QuadFindError):
        det.detect(torch.zeros((1, 48, 64), dtype=torch.uint8), min_area=2 ** 40)
    for frames in (torch.zeros((1, 48, 64), dtype=torch.uint8), np.zeros((1, 48, 64), np.uint8), torch.zeros((48, 64), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="cuda u8"):
            det.detect(frames)
        with pytest.raises(ValueError, match="cuda u8"):
            det.labels(frames)
    with pytest.raises(ValueError, match="tag_ids"):
        tag_detect.family_lut(tag_decode.TagFamily(ts.family_codes()), [0, 1, 1], 3, "cpu")
    with pytest.raises(ValueError, match="tag_ids"):
        tag_detect.family_lut(tag_decode.TagFamily(ts.family_codes()), [0, 1, ts.N_CODES], 3, "cpu")
    assert tag_detect.family_lut(tag_decode.TagFamily(ts.family_codes()), [5, 3], 2, "cpu").tolist()[:6] == [-1, -1, -1, 1, -1, 0]
    with pytest.raises(ValueError):
        tag_detect.DeviceTagDetector(tag_decode.TagFamily(ts.family_codes()), min_contrast="x")


def test_argument_errors_of_the_library_need_no_device():
    """every refusal comes before any device work: creation is refused by value, and so are calls on no handle"""
    import ctypes as C
    from accurate_aprilgroup_tracking_amd import quadfindlib as Q
    L = Q.lib()
    h = C.c_void_p()
    for args in ((7, 48, 1, 16, 8), (64, 7, 1, 16, 8), (Q.MAX_SIZE + 1, 48, 1, 16, 8), (64, 48, 0, 16, 8), (64, 48, Q.MAX_BATCH + 1, 16, 8),
                 (64, 48, 1, 0, 0), (64, 48, 1, 16, 17), (64, 48, 1, Q.MAX_COMPONENTS + 1, 8)):
        assert L.agt_quadfind_create(*args, C.byref(h)) == Q.ERR_ARG and not h.value, args
    assert L.agt_quadfind_create(64, 48, 1, 16, 8, None) == Q.ERR_ARG
    assert L.agt_quadfind_destroy(None) == Q.ERR_ARG
    assert L.agt_quadfind_detect(None, None, 64, 64, 64 * 48, 64, 48, 1, None, 64, 64, 64) == Q.ERR_ARG
    assert L.agt_quadfind_labels(None, None, 64, 64, 64 * 48, 64, 48, 1, 40, 64) == Q.ERR_ARG
